"""Device-side batch construction: raw trajectories -> padded `Batch1` on the GPU in one pass.

This is the default data path of the trainer / bench.  It replaces the per-sample
`wrapper.preprocess_item` + `algos` calls and the per-batch `collator_*` of the reference
(`wrapper.py:25-102`, `collator.py:310-458`) with: one host-side packing of the raw dicts
(`gen_pickles.py:820-832` format) into padded arrays, one H2D copy each, `mobgt_spd_batched` for
SPD / path / first-D-hop edge features / degrees, and a gather from a precomputed distance-bin table for
`poi_pos`.  Index tensors stay narrow on the device (int16 / uint8 instead of the reference's int64):
the kernels are templated on the index type, and `.long()` views give the reference dtypes when needed.
Every field equals what the reference pipeline produces for the same trajectories
(tests/test_gpu_model.py::test_device_collator_matches_reference_batch, tests/test_gpu_pair_bins.py).
"""
import collections

import numpy as np
import torch

from . import ops
from .collator import Batch1, freedman_diaconis_bins


def make_bin_table(distance, dtype=np.int16):
    """(P+1)x(P+1) distance matrix -> (num_bins, bin ids): bin[a,b] = np.digitize(distance[a,b], edges) with the
    Freedman-Diaconis edges of collator.py:430-433.  Computed once instead of per batch."""
    d = np.asarray(distance)
    dm = np.delete(np.delete(d, 0, axis=0), 0, axis=1)
    num_bins, edges = freedman_diaconis_bins(dm - dm.min(), True)
    return num_bins, edges, np.digitize(d, edges).astype(dtype)


class DeviceBatch1(Batch1):
    """`Batch1` whose model-unused fields (adj, adj1, attn_edge_type, feature_matrix) are derived on first
    access from the packed counts, so the hot path does not pay for them."""
    _fields = ("idx", "attn_bias", "rel_pos", "in_degree", "out_degree", "x", "edge_input", "y", "time", "time_normal",
               "user", "cat", "poi_pos")

    def __init__(self, counts, n_nodes, **kw):
        for f in self._fields:
            setattr(self, f, kw[f])
        self._feature_matrix = None
        self._counts, self._n_nodes = counts, n_nodes

    def to(self, device):
        for f in self._fields:
            setattr(self, f, getattr(self, f).to(device))
        self._counts, self._n_nodes = self._counts.to(device), self._n_nodes.to(device)
        return self

    @property
    def adj1(self):                                                   # wrapper.py:73-76, collator.py:386
        return self._counts != 0

    @property
    def adj(self):                                                    # wrapper.py:67-81, collator.py:384
        G, N = self._counts.shape[:2]
        a = torch.zeros(G, N + 1, N + 1, dtype=torch.bool, device=self._counts.device)
        a[:, :N, :N] = self._counts != 0
        ar = torch.arange(N + 1, device=a.device)
        n = self._n_nodes.long().view(G, 1)
        inside = ar.view(1, -1) <= n                                  # positions 0..n of each graph
        tok = ar.view(1, -1) == n                                     # the virtual token sits at index n
        a |= tok.unsqueeze(2) & inside.unsqueeze(1)
        a |= inside.unsqueeze(2) & tok.unsqueeze(1)
        return a

    @property
    def attn_edge_type(self):                                         # wrapper.py:49-53, collator.py:412-417
        G, N = self._counts.shape[:2]
        t = torch.zeros(G, N + 1, N + 1, 1, dtype=torch.long, device=self._counts.device)
        c = self._counts.long()
        t[:, :N, :N, 0] = torch.where(c != 0, c + 2, c)
        return t


class DeviceCollator:
    """callable(list of raw trajectory dicts) -> DeviceBatch1 on `device`.
    Mirrors `partial(collator_foursquare, max_node=30000, multi_hop_max_dist=D, rel_pos_max=R)` (data.py:289-294)
    applied to `preprocess_item`-ed items."""

    def __init__(self, device, bin_table=None, multi_hop_max_dist=20, rel_pos_max=1024, max_node=30000, coords=None,
                 bin_edges=None, pair_bins=None):
        """`bin_table`: (P+1) x (P+1) precomputed distance-bin ids (make_bin_table).  For universes where that table
        cannot exist (P = 100 000), `coords` [(P+1), 2] lat / lon + `bin_edges`: poi_pos = digitize(haversine) is then
        evaluated for the batch's pairs on the device with torch ops.  `pair_bins` (geo.pair_bins), instead of either: poi_pos
        is the search of the pairs' squared chords among the edges as squared chords, one launch (mobgt_bins_batch) beside
        mobgt_collate_finish, so the collate can run on a loop's copy stream (can_finish_into); `coords` given with it only
        serves as the default coordinates of recommend / evaluate(within_km=)."""
        if pair_bins is not None and (bin_table is not None or bin_edges is not None):
            raise ValueError("DeviceCollator: pair_bins= replaces bin_table= and bin_edges=, give one of them")
        self.device = torch.device(device)
        self.D = int(multi_hop_max_dist)
        self.rel_pos_max = int(rel_pos_max)
        self.max_node = int(max_node)
        self.bin_table = None
        if bin_table is not None:
            self.bin_table = torch.as_tensor(bin_table).to(self.device)
        self.coords = self.bin_edges = None
        if coords is not None:
            self.coords = torch.as_tensor(np.radians(np.asarray(coords, dtype=np.float64))).to(self.device)
            if pair_bins is None:
                self.bin_edges = torch.as_tensor(np.asarray(bin_edges, dtype=np.float64)).to(self.device)
        self.pair_bins = pair_bins.to(self.device) if pair_bins is not None else None
        # where poi_pos comes from, decided once: the chord search, the table, haversine + bucketize, or nowhere (all zeros)
        self.poi_source = ("pair_bins" if pair_bins is not None else "table" if bin_table is not None
                           else "haversine" if coords is not None else None)

    def pack_host(self, trajs, idx0=0, n_pad=None, out=None):
        """Raw dicts -> padded numpy arrays (pinned-memory friendly); no graph algorithm runs on the host.
        `n_pad`: pad to this many nodes instead of the batch maximum (bucketed shapes: the extra positions are padding
        exactly like the collator's own, collator.py:11-101); `out`: pre-allocated arrays to fill (RawLayout.views)."""
        trajs = [t for t in trajs if t is not None and len(t["node_name"]) <= self.max_node]
        G = len(trajs)
        n = np.array([len(t["node_name"]) for t in trajs], dtype=np.int32)
        N = int(n.max()) if n_pad is None else int(n_pad)
        if N < int(n.max()):
            raise ValueError(f"n_pad {N} is smaller than the longest trajectory ({int(n.max())})")
        if out is not None:
            for k in ("counts", "x", "time", "cat", "time_normal"):
                out[k][...] = 0
            counts, x, time, cat, time_normal = out["counts"], out["x"], out["time"], out["cat"], out["time_normal"]
            assert counts.shape == (G, N, N), (counts.shape, G, N)
        else:
            counts = np.zeros((G, N, N), dtype=np.int32)
            x = np.zeros((G, N, 1), dtype=np.int32)
            time = np.zeros((G, N, 1), dtype=np.int32)
            cat = np.zeros((G, N, 1), dtype=np.int32)
            time_normal = np.zeros((G, N, 1), dtype=np.float32)
        for g, t in enumerate(trajs):
            k = n[g]
            counts[g, :k, :k] = t["edge_type"]
            x[g, :k, 0] = t["node_name"]                              # wrapper +1 then collator -1 (App. A)
            time[g, :k, 0] = t["time"]
            cat[g, :k, 0] = t["cat"]
            time_normal[g, :k, 0] = t["time_normal"]
        user = np.array([[int(t["user"][0]) + 1] for t in trajs], dtype=np.int32)       # wrapper.py:39
        y = np.array([int(t["target"][0]) for t in trajs], dtype=np.int64)              # collator.py:367
        idx = np.arange(idx0, idx0 + G, dtype=np.int64) if np.isscalar(idx0) else np.asarray(idx0, dtype=np.int64)
        if out is not None:
            out["n_nodes"][...], out["user"][...], out["y"][...], out["idx"][...] = n, user, y, idx
            return out
        return dict(counts=counts, n_nodes=n, x=x, time=time, cat=cat, time_normal=time_normal, user=user, y=y, idx=idx)

    def __call__(self, trajs, idx0=0, n_pad=None):
        h = self.pack_host(trajs, idx0, n_pad=n_pad)
        d = {k: torch.from_numpy(v).to(self.device, non_blocking=True) for k, v in h.items()}
        return self.finish(d)

    # ---- what the loops over fresh batches (train._StagedBatches) ask of a collator: the input form is the collator's business.
    # Here: trajectory dicts, staged as RawLayout's arrays.  SessionCollator overrides these for check-in sessions.
    def nodes_of(self, sample):
        """Node count of one sample of the dataset (what its batch's bucket is chosen by)."""
        return len(sample["node_name"])

    def keeps(self, sample):
        """Whether a sample enters a batch: longer ones than max_node are dropped (as the reference's collator does)."""
        return sample is not None and self.nodes_of(sample) <= self.max_node

    @staticmethod
    def lengths_of(dataset):
        """Node counts of a whole dataset (data.balanced_batches deals by them)."""
        return [len(t["node_name"]) for t in dataset]

    def new_stage(self, lay, side, host=True):
        """One staging buffer pair of a (G, N) bucket: a pinned host buffer for the raw part and a device buffer of the whole
        layout (`side`: with the derived fields, whose views finish_into fills)."""
        raw_bytes = lay.raw_bytes if side else lay.nbytes
        dev = torch.zeros(lay.nbytes, dtype=torch.uint8, device=self.device)
        st = dict(pin=None, np=None, dev=dev, dev_views=lay.views_torch(dev) if side else None, work=None,
                  ready=torch.cuda.Event(), free=None, used=False, index=None, batch=None, layout=lay, raw_bytes=raw_bytes)
        if host:
            self._host_stage(st)
        return st

    @staticmethod
    def _host_stage(st):
        st["pin"] = torch.zeros(st["raw_bytes"], dtype=torch.uint8).pin_memory()
        st["np"] = st["layout"].views_np(st["pin"].numpy())

    def stage_host(self, st, samples, idx0, N):
        """Host half of staging a batch: the samples into the stage's pinned buffer -> the host arrays limit_violation reads."""
        return self.pack_host(samples, idx0=idx0, n_pad=N, out=st["np"])

    def limit_violation(self, h, L):
        """The first field of stage_host's arrays that holds an index outside the model's tables (L = model.index_limits()):
        (field, index, table rows), or None.  Checked on the host, before anything is launched."""
        bad = self._id_violation(h["x"], h, L)
        if bad:
            return bad
        nz = h["counts"] != 0
        if "edge" in L and int(h["counts"].max()) + 3 >= L["edge"]:
            return "edge_input", int(h["counts"].max()) + 3, L["edge"]
        if "deg" in L and max(int(nz.sum(1).max()), int(nz.sum(2).max())) + 1 >= L["deg"]:
            return "degree", max(int(nz.sum(1).max()), int(nz.sum(2).max())) + 1, L["deg"]
        if "slots" in L and int(float(h["time_normal"].max()) * 48) >= L["slots"]:
            return "time_normal", float(h["time_normal"].max()), L["slots"]
        return None

    @staticmethod
    def _id_violation(x, h, L):
        """limit_violation's first three checks -- POI ids `x` (the dict form's h["x"], the session form's check-in column),
        h["user"], h["y"] -- in that order."""
        for field, ids in (("x", x), ("user", h["user"]), ("y", h["y"])):
            if field in L and int(ids.max()) > L[field]:
                return field, int(ids.max()), L[field] + 1
        return None

    def upload(self, st):
        """Device half, on the CURRENT stream (the loop's copy stream): the staged host bytes -> the raw fields of st["dev"]."""
        st["dev"][:st["pin"].numel()].copy_(st["pin"], non_blocking=True)

    def can_finish_into(self):
        """Whether finish_into's launches give this collator's poi_pos: the chord search, mobgt_collate_finish's gather from a
        contiguous int16 table, or its zeros.  Haversine bins, and any other table, need finish's torch form."""
        if self.poi_source == "table":                                # (a table beside coords= keeps the torch form)
            return self.coords is None and self.bin_table.dtype == torch.int16 and self.bin_table.is_contiguous()
        return self.poi_source != "haversine"

    def finish_into(self, v, work=None):
        """`finish` writing into the pre-allocated views of a BatchLayout buffer (raw fields already in place): two / three
        launches on the CURRENT stream (one more with pair_bins), no allocation -- train.EpochLoop runs it on its copy stream for
        the next batch."""
        from . import _lib, geo
        from .ops import _p, _stream
        G, N = v["counts"].shape[:2]
        lib = _lib.lib()
        if work is None:
            work = torch.empty(int(lib.mobgt_spd_workspace_bytes(G, N)), dtype=torch.uint8, device=self.device)
        _lib.call("mobgt_spd_batched", _p(v["counts"]), _p(v["n_nodes"]), _p(v["spd"]), _p(v["path"]), _p(v["rel_pos"]),
                  _p(v["edge_input"]), _p(v["in_degree"]), _p(v["out_degree"]), _p(work), G, N, self.D,
                  _stream())
        bt = self.bin_table
        _lib.call("mobgt_collate_finish", _p(v["x"]), _p(v["n_nodes"]), _p(v["spd"]), _p(bt), bt.shape[1] if bt is not None else 0,
                  self.rel_pos_max, _p(v["attn_bias"]), _p(v["poi_pos"]), G, N, _stream())
        if self.poi_source == "pair_bins":
            geo.batch_bins(self.pair_bins, v["x"], out=v["poi_pos"])
        return work

    @staticmethod
    def batch_from_views(v):
        return DeviceBatch1(v["counts"], v["n_nodes"], **{f: v[f] for f in DeviceBatch1._fields})

    def finish(self, d):
        """Raw device arrays (pack_host's names) -> DeviceBatch1.  finish_into's launches into freshly allocated tensors when they
        give this collator's poi_pos and the arrays are what the kernels read; the torch-op form otherwise."""
        ops._require_cuda(d["counts"], d["n_nodes"])
        if not (self.can_finish_into() and all(d[k].dtype == torch.int32 and d[k].is_contiguous() for k in ("counts", "x", "n_nodes"))):
            return self._finish_torch(d)
        G, N = d["counts"].shape[:2]
        v = dict(d)
        for name, dt, shape in BatchLayout.DERIVED + BatchLayout.SCRATCH:
            v[name] = torch.empty(shape(G, N, self.D), dtype=TORCH_DTYPE[dt], device=self.device)
        self.finish_into(v)
        return self.batch_from_views(v)

    def _finish_torch(self, d):
        """finish in torch ops behind mobgt_spd_batched: for haversine bins, a table that is not contiguous int16, ids of
        another dtype."""
        n_nodes, x = d["n_nodes"], d["x"]
        G, N = d["counts"].shape[:2]
        T = N + 1
        sp = ops.spd_batched(d["counts"], n_nodes, self.D)
        ar = torch.arange(T, device=self.device)
        real_tok = ar.view(1, T) <= n_nodes.view(G, 1)                # token 0 + n real nodes
        attn_bias = torch.zeros(G, T, T, device=self.device)
        attn_bias.masked_fill_(~real_tok.view(G, 1, T), float("-inf"))              # collator.py:57-64
        if self.rel_pos_max <= 510:                                                  # collator.py:354-358
            far = sp["spd"] >= self.rel_pos_max
            attn_bias[:, 1:, 1:].masked_fill_(far, float("-inf"))
        if self.poi_source == "pair_bins":                                           # (the same launch: it zeroes the pad pairs)
            from . import geo
            poi_pos = geo.batch_bins(self.pair_bins, x[:, :, 0].to(torch.int32).contiguous())
        elif self.poi_source is None:
            poi_pos = torch.zeros(G, N, N, dtype=torch.int16, device=self.device)
        else:
            xi = x[:, :, 0].long()
            if self.poi_source == "table":
                poi_pos = self.bin_table[xi.unsqueeze(2), xi.unsqueeze(1)]
            else:
                ll = self.coords[xi]                                                 # [G,N,2] radians, float64
                lat1, lon1, lat2, lon2 = ll[:, :, None, 0], ll[:, :, None, 1], ll[:, None, :, 0], ll[:, None, :, 1]
                h = torch.sin((lat2 - lat1) / 2) ** 2 + torch.cos(lat1) * torch.cos(lat2) * torch.sin((lon2 - lon1) / 2) ** 2
                dist = 2 * 6371.0 * torch.asin(torch.sqrt(h.clamp(0.0, 1.0)))      # synth.haversine_km
                poi_pos = torch.bucketize(dist, self.bin_edges, right=True).to(torch.int16)   # == np.digitize(dist, edges)
            real = xi != 0
            poi_pos = torch.where(real.unsqueeze(2) & real.unsqueeze(1), poi_pos, torch.zeros_like(poi_pos))
        return self.batch_from_views(dict(d, attn_bias=attn_bias, poi_pos=poi_pos, **sp))


# ---- bucketed shapes for a loop over FRESH batches (train.TrainStep.run_epoch) ------------------------------------------------
# A hipGraph has static shapes, and the reference feeds a new batch every step (data.py:282-295): the padded node count of
# a batch is therefore rounded UP to one of a few sizes and one step graph is kept per (G, size).  Rounding up only adds
# padding positions, which the collator already produces for every graph shorter than the batch maximum (-inf key columns,
# zero indices): logits, loss and gradients do not change (tests/test_gpu_loop.py).
# (round 4: steps of 1/16 .. 1/8 of the size instead of round 3's 1/3 .. 1/2 (8, 16, 24, 32, 48, 64, 96, ...): at most ~6-12 % of
#  padding in N instead of ~33 %.  A bucket costs one captured step graph, taken the first time it occurs.  Measured on the
#  S-FSQ pool: fresh-batch loop 0.784 -> 0.700 ms per step with steps of 1/8 .. 1/4)
BUCKETS = (tuple(range(4, 65, 4)) + tuple(range(72, 129, 8)) + tuple(range(144, 257, 16)) + tuple(range(288, 513, 32))
           + tuple(range(576, 1025, 64)))


def balanced_batches(lengths, world_size, batch_size, epoch=0, seed=0, shuffle=True, buckets=BUCKETS, window=None):
    """Length-balanced dealing of one epoch over `world_size` ranks ("load imbalance across ranks": node
    counts run from 1 to 814 on Gowalla, a step costs what its padded N costs, and a synchronous step lasts as long as its
    slowest rank): -> steps[j][r] = sample ids of rank r in step j, the same list on every rank.

    * the epoch's samples are exactly DistributedSampler's (`shard_indices`): the permutation seeded by seed + epoch, padded by
      wrap-around to a multiple of world_size -- the union over ranks is the same multiset, every rank takes the same number of
      samples and of steps, the last step is the short one on all ranks alike (drop_last=False, data.py:282-295);
    * inside it the samples are ordered by the BUCKET their node count pads to (stable: samples of one bucket keep their random
      order, so a batch's composition stays random) and cut into steps of world_size x batch_size; rank r takes the r-th run of a
      step -- neighbouring runs of one sorted sequence, i.e. the same or the neighbouring bucket on all ranks;
    * the steps are then visited in an order drawn from seed + epoch + 1 (sizes mixed over time: the learning-rate schedule
      never sees 'all short graphs first');
    * `window` (steps; None = the whole epoch): the sort runs inside consecutive windows of window x world_size x batch_size
      samples of the permuted epoch only -- every window is a uniform random sample of the dataset, so a step's batches are
      length-homogeneous only with respect to the ~window x world x batch samples around them, and the long graphs of an epoch are
      spread over its windows instead of sharing one step (whole-epoch sorting changes SGD's batch statistics against
      the reference's i.i.d. DistributedSampler batches; `train.EpochLoop` therefore uses a bounded window by default)."""
    n = len(lengths)
    if shuffle:
        g = torch.Generator()
        g.manual_seed(seed + epoch)
        order = torch.randperm(n, generator=g).tolist()
    else:
        order = list(range(n))
    total = (n + world_size - 1) // world_size * world_size
    order += order[: total - len(order)]
    per_step = world_size * batch_size
    span = total if window is None else max(1, int(window)) * per_step
    steps = []
    for w0 in range(0, total, span):
        keyed = sorted(order[w0:w0 + span], key=lambda i: bucket_nodes(int(lengths[i]), buckets))          # (stable)
        for s in range(0, len(keyed), per_step):
            chunk = keyed[s:s + per_step]
            m = len(chunk) // world_size                                                 # (total is a multiple of world_size)
            steps.append([chunk[r * m:(r + 1) * m] for r in range(world_size)])
    # (windows: only the epoch's LAST step can be short -- every window but the last holds whole steps)
    if shuffle:
        g = torch.Generator()
        g.manual_seed(seed + epoch + 1)
        steps = [steps[i] for i in torch.randperm(len(steps), generator=g).tolist()]
    return steps


def bucket_nodes(n, buckets=BUCKETS):
    """Smallest bucket >= n (beyond the largest: the next multiple of 256)."""
    for b in buckets:
        if n <= b:
            return b
    return (n + 255) // 256 * 256


TORCH_DTYPE = {np.int64: torch.int64, np.int32: torch.int32, np.float32: torch.float32, np.int16: torch.int16, np.uint8: torch.uint8}


class RawLayout:
    """The raw (un-collated) arrays of one (G, N) bucket packed into ONE byte buffer, so that a step's input is one
    host-to-device copy: 8-byte fields first, every field 16-byte aligned."""
    FIELDS = (("y", np.int64, lambda G, N, D: (G,)), ("idx", np.int64, lambda G, N, D: (G,)),
              ("counts", np.int32, lambda G, N, D: (G, N, N)), ("x", np.int32, lambda G, N, D: (G, N, 1)),
              ("time", np.int32, lambda G, N, D: (G, N, 1)), ("cat", np.int32, lambda G, N, D: (G, N, 1)),
              ("time_normal", np.float32, lambda G, N, D: (G, N, 1)), ("n_nodes", np.int32, lambda G, N, D: (G,)),
              ("user", np.int32, lambda G, N, D: (G, 1)))

    def __init__(self, G, N, D=0):
        self.G, self.N, self.D = int(G), int(N), int(D)
        self.offsets = {}
        self.nbytes = self.raw_bytes = self._place(self.FIELDS, 0)

    def _place(self, fields, off):
        """Append `fields` to the layout from byte `off` on -> the (16-byte aligned) end."""
        for name, dt, shape in fields:
            shp = shape(self.G, self.N, self.D)
            nbytes = int(np.prod(shp)) * np.dtype(dt).itemsize
            self.offsets[name] = (off, nbytes, dt, shp)
            off = (off + nbytes + 15) // 16 * 16
        return off

    def views_np(self, buf):
        """numpy views of the RAW part of a host uint8 array (e.g. `pinned_tensor.numpy()`, a staging buffer of raw_bytes)"""
        return {k: buf[o:o + n].view(dt).reshape(shp) for k, (o, n, dt, shp) in self.offsets.items() if o + n <= self.raw_bytes}

    def views_torch(self, buf):
        """typed torch views of a (device) uint8 tensor"""
        return {k: buf[o:o + n].view(TORCH_DTYPE[dt]).view(*shp) for k, (o, n, dt, shp) in self.offsets.items()}


class BatchLayout(RawLayout):
    """RawLayout + everything the device collate derives from it, in one byte buffer: [raw fields | derived fields |
    scratch].  A staging copy of this buffer is filled on a side stream (H2D of the raw part, then the collate kernels)
    while the previous step runs; ONE device-to-device copy of [raw | derived] then refreshes the static buffer the bucket's
    step graph reads.  DERIVED and SCRATCH are also what DeviceCollator.finish allocates, as tensors of their own."""
    DERIVED = (("attn_bias", np.float32, lambda G, N, D: (G, N + 1, N + 1)), ("rel_pos", np.int16, lambda G, N, D: (G, N, N)),
               ("poi_pos", np.int16, lambda G, N, D: (G, N, N)), ("edge_input", np.uint8, lambda G, N, D: (G, N, N, D, 1)),
               ("in_degree", np.int16, lambda G, N, D: (G, N)), ("out_degree", np.int16, lambda G, N, D: (G, N)))
    SCRATCH = (("spd", np.int16, lambda G, N, D: (G, N, N)), ("path", np.int16, lambda G, N, D: (G, N, N)))

    def __init__(self, G, N, D):
        super().__init__(G, N, D)
        self.copy_bytes = self._place(self.DERIVED, self.raw_bytes)   # [raw | derived]: what a step's graph reads
        self.nbytes = self._place(self.SCRATCH, self.copy_bytes)


def shard_indices(n_samples, rank, world_size, epoch=0, seed=0, shuffle=True):
    """torch DistributedSampler semantics (what Lightning's DDP uses, entry.py:141): permutation seeded by
    seed+epoch, padded by wrap-around to a multiple of world_size, strided by rank."""
    if shuffle:
        g = torch.Generator()
        g.manual_seed(seed + epoch)
        order = torch.randperm(n_samples, generator=g).tolist()
    else:
        order = list(range(n_samples))
    total = (n_samples + world_size - 1) // world_size * world_size
    order += order[: total - len(order)]
    return order[rank:total:world_size]


# ---- check-in sessions as the input form ----------------------------------------------------------------------------------------
# What a user has, and what a recommender is served with, is a session: a user id and a visit-ordered list of check-ins, the
# last one the target.  The reference turns sessions into the trajectory dicts above with a pandas loop
# (gen_pickles.py:735-833); here sessions_to_trajectories does it in numpy (the host reference, the offline converter and the
# fall-back) and SessionCollator on the device (csrc_data/sessions.hip through _lib_data).
SessionRecord = collections.namedtuple("SessionRecord", "user checkins n mult")
SessionRecord.__doc__ = """One session of a SessionDataset: user id, checkins [L + 1, 3] int32 rows (poi, time slot, category) in visit
order (the last row is the target), n = distinct POIs of the history checkins[:L], mult = how often its most visited POI occurs."""


def session_graph(hist):
    """History check-ins [L, 3] (poi, time slot, category) in visit order -> the graph fields of gen_pickles.py:755-832:
    nodes are the distinct POIs ordered by their LAST occurrence (:789-791 drop_duplicates(keep='last')), so node n - 1 is the
    last check-in's POI; edge_type[a, b] counts the transitions a -> b (:783-785), self transitions on the diagonal, nothing
    clipped; time / cat are the values at the node's last occurrence (:786-787); time_normal = 0 for slot 0, else
    float32(time / 48) with a double quotient (:805-809, :828)."""
    hist = np.asarray(hist)
    poi = hist[:, 0].astype(np.int64)
    L = len(poi)
    uniq, first_rev, inv = np.unique(poi[::-1], return_index=True, return_inverse=True)
    last = L - 1 - first_rev                                          # last position of every distinct POI (in POI order)
    order = np.argsort(last)
    pos = last[order]                                                 # the nodes' positions, ascending
    rank = np.empty(len(uniq), dtype=np.int64)
    rank[order] = np.arange(len(uniq))
    node = rank[inv.reshape(-1)[::-1]]                                # node index of every check-in
    edge = np.zeros((len(uniq), len(uniq)), dtype=np.int64)
    np.add.at(edge, (node[:-1], node[1:]), 1)
    time = hist[pos, 1].astype(np.int64)
    with np.errstate(divide="ignore"):
        time_normal = np.where(time == 0, 0.0, time / 48).astype(np.float32)
    return dict(node_name=poi[pos], edge_type=edge, time=time, time_normal=time_normal, cat=hist[pos, 2].astype(np.int64))


def _validated(s, what):
    """(user, checkins) -> (user, integer array [L + 1, 3] whose values fit int32), or ValueError naming `what`."""
    try:
        user, checkins = s
    except (TypeError, ValueError):
        raise ValueError(f"{what}: expected (user, checkins)") from None
    c = np.asarray(checkins)
    if c.ndim != 2 or c.shape[1] != 3:
        raise ValueError(f"{what}: checkins must be [L + 1, 3] rows of (poi, time slot, category), got shape {c.shape}")
    if c.shape[0] < 2:
        raise ValueError(f"{what} has {c.shape[0]} check-in(s): a history of at least one and a target are needed")
    if not np.issubdtype(c.dtype, np.integer) or not isinstance(user, (int, np.integer)):
        raise ValueError(f"{what}: user and checkins must be integers (got {type(user).__name__}, {c.dtype})")
    if c.min() < np.iinfo(np.int32).min or c.max() > np.iinfo(np.int32).max:
        raise ValueError(f"{what}: a value does not fit int32")
    return int(user), c


def _as_record(s, what="a session"):
    """A SessionRecord passes (its dataset validated it); a raw (user, checkins) pair is validated as SessionDataset does."""
    if isinstance(s, SessionRecord):
        return s
    user, c = _validated(s, what)
    _, cnt = np.unique(c[:-1, 0], return_counts=True)
    return SessionRecord(user, c, len(cnt), int(cnt.max()))


def sessions_to_trajectories(sessions):
    """Sessions -- (user, checkins [L + 1, 3]) pairs, SessionRecords or a SessionDataset -- -> the list of trajectory dicts in
    the gen_pickles.py:820-832 format (numpy arrays, as synth.make_trajectory's): what gen_poigraph_d1228_nyc_avg_maxtime
    writes for them, field by field and bit by bit (tests/test_host_sessions.py, golden G12)."""
    out = []
    for s in sessions:
        r = _as_record(s)
        c = np.asarray(r.checkins)
        d = session_graph(c[:-1])
        d["target"] = np.array([int(c[-1, 0])], dtype=np.int64)       # :761, :824
        d["user"] = np.array([int(r.user)], dtype=np.int64)           # :829
        out.append(d)
    return out


class SessionDataset:
    """A dataset of sessions for SessionCollator and the loops: validated once, stored packed (one [sum(L + 1), 3] int32 array
    plus offsets), with every session's n (distinct POIs of its history: what buckets and max_node go by) and the largest
    multiplicity of a POI in it (a bound on its edge counts).  ds[i] is a light SessionRecord over views of the packed array."""

    def __init__(self, sessions):
        users, rows, offs, n, mult = [], [], [0], [], []
        for i, s in enumerate(sessions):
            user, c = _validated(s, f"session {i}")
            _, cnt = np.unique(c[:-1, 0], return_counts=True)
            users.append(user)
            rows.append(c.astype(np.int32))
            offs.append(offs[-1] + c.shape[0])
            n.append(len(cnt))
            mult.append(int(cnt.max()))
        self.seq = np.concatenate(rows) if rows else np.zeros((0, 3), dtype=np.int32)
        self.offsets = np.asarray(offs, dtype=np.int64)
        self.users = np.asarray(users, dtype=np.int64)
        self.n = np.asarray(n, dtype=np.int32)
        self.mult = np.asarray(mult, dtype=np.int32)

    @classmethod
    def from_packed(cls, seq, offsets, users, n, mult):
        """The dataset of arrays that are packed already (checkins.sessionize builds them on the device; the constructor's loop
        over sessions would not do for 10^5 of them): validated vectorised, stored as they come.  seq [M, 3] int32, offsets
        [S + 1] ascending from 0 to M with at least two rows per session, users [S], n / mult [S] as the constructor computes
        them (1 <= n, mult <= history rows; taken on trust beyond that)."""
        seq, offsets, users, n, mult = (np.asarray(a) for a in (seq, offsets, users, n, mult))
        for name, a in (("seq", seq), ("offsets", offsets), ("users", users), ("n", n), ("mult", mult)):
            if a.size and not np.issubdtype(a.dtype, np.integer):
                raise ValueError(f"SessionDataset.from_packed: {name} must be integers, got {a.dtype}")
        if seq.ndim != 2 or seq.shape[1] != 3:
            raise ValueError(f"SessionDataset.from_packed: seq must be [M, 3] rows of (poi, time slot, category), got shape {seq.shape}")
        if seq.size and (seq.min() < np.iinfo(np.int32).min or seq.max() > np.iinfo(np.int32).max):
            raise ValueError("SessionDataset.from_packed: a value of seq does not fit int32")
        S = len(users)
        if offsets.shape != (S + 1,) or users.ndim != 1 or n.shape != (S,) or mult.shape != (S,):
            raise ValueError(f"SessionDataset.from_packed: {S} users need offsets [{S + 1}], n [{S}] and mult [{S}], got "
                             f"{offsets.shape}, {n.shape}, {mult.shape}")
        lengths = np.diff(offsets)
        if int(offsets[0]) != 0 or int(offsets[-1]) != seq.shape[0]:
            raise ValueError(f"SessionDataset.from_packed: offsets run from {int(offsets[0])} to {int(offsets[-1])}, seq has {seq.shape[0]} rows")
        if S and lengths.min() < 2:
            s = int(np.argmax(lengths < 2))
            raise ValueError(f"session {s} has {int(lengths[s])} check-in(s): a history of at least one and a target are needed")
        if S and ((n < 1) | (n > lengths - 1) | (mult < 1) | (mult > lengths - 1)).any():
            s = int(np.argmax((n < 1) | (n > lengths - 1) | (mult < 1) | (mult > lengths - 1)))
            raise ValueError(f"session {s}: n = {int(n[s])} / mult = {int(mult[s])} for a history of {int(lengths[s]) - 1} check-in(s)")
        self = cls.__new__(cls)
        self.seq = np.ascontiguousarray(seq, dtype=np.int32)
        self.offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        self.users = np.ascontiguousarray(users, dtype=np.int64)
        self.n = np.ascontiguousarray(n, dtype=np.int32)
        self.mult = np.ascontiguousarray(mult, dtype=np.int32)
        return self

    def __len__(self):
        return len(self.users)

    def __getitem__(self, i):
        i = int(i)
        if not -len(self) <= i < len(self):
            raise IndexError(i)
        i %= len(self)
        return SessionRecord(int(self.users[i]), self.seq[self.offsets[i]:self.offsets[i + 1]], int(self.n[i]), int(self.mult[i]))

    @property
    def max_n(self):
        """The longest trajectory graph of the dataset (nodes)."""
        return int(self.n.max()) if len(self) else 0


class SessionLayout:
    """What travels to the device for a batch of sessions, in ONE byte buffer: y and idx at RawLayout's offsets (one device
    copy moves both), then user, len and seq [G, Lp, 3]; every field 16-byte aligned."""

    def __init__(self, G):
        self.G = G = int(G)
        a16 = lambda v: (v + 15) // 16 * 16
        self.idx_off = a16(8 * G)
        self.head_bytes = self.idx_off + 8 * G                        # [y | idx]: RawLayout's first two fields, same offsets
        self.user_off = a16(self.head_bytes)
        self.len_off = self.user_off + a16(4 * G)
        self.seq_off = self.len_off + a16(4 * G)
        assert RawLayout(G, 1).offsets["idx"][0] == self.idx_off and RawLayout(G, 1).offsets["y"][0] == 0

    def nbytes(self, Lp):
        return self.seq_off + (12 * self.G * int(Lp) + 15) // 16 * 16

    def views_np(self, buf, Lp):
        G = self.G
        return dict(y=buf[:8 * G].view(np.int64), idx=buf[self.idx_off:self.idx_off + 8 * G].view(np.int64),
                    user=buf[self.user_off:self.user_off + 4 * G].view(np.int32).reshape(G, 1),
                    len=buf[self.len_off:self.len_off + 4 * G].view(np.int32),
                    seq=buf[self.seq_off:self.seq_off + 12 * G * Lp].view(np.int32).reshape(G, Lp, 3))


class SessionCollator(DeviceCollator):
    """callable(list of sessions or SessionRecords) -> the DeviceBatch1 DeviceCollator returns for the converted dicts
    (sessions_to_trajectories): seq / len / user / y / idx are packed on the host and copied in one piece, the raw graph
    fields are built on the device (mobgt_sessions_to_raw, include/mobgt_data.h) straight into RawLayout's views, then the
    existing finish.  The constructor is DeviceCollator's.  A batch beyond the kernel's limits (history longer than
    _lib_data.MAX_LP, padded N over _lib_data.MAX_N) is converted on the host and takes DeviceCollator's path.

    The host checks what the kernel would refuse (lengths, node counts against n_pad), so the kernel's per-graph status is
    not read back on this path."""

    # ---- host packing ---------------------------------------------------------------------------------------------------
    @staticmethod
    def pack_sessions(recs, idx0, v):
        """Records -> the numpy views of a SessionLayout buffer (padding rows of seq zeroed: the whole buffer is copied)."""
        for g, r in enumerate(recs):
            L = len(r.checkins) - 1
            v["seq"][g, :L] = r.checkins[:L]
            v["seq"][g, L:] = 0
            v["len"][g] = L
            v["user"][g, 0] = r.user + 1                              # wrapper.py:39
            v["y"][g] = r.checkins[L, 0]                              # collator.py:367
        G = len(recs)
        v["idx"][...] = np.arange(idx0, idx0 + G, dtype=np.int64) if np.isscalar(idx0) else np.asarray(idx0, dtype=np.int64)
        v["n"] = np.array([r.n for r in recs], dtype=np.int32)
        v["recs"] = recs
        return v

    @staticmethod
    def fits_kernel(Lp, N):
        from . import _lib_data
        return Lp <= _lib_data.MAX_LP and N <= _lib_data.MAX_N

    def to_raw(self, sdev, slay, Lp, buf, raw, status):
        """On the current stream: the session bytes on the device (a SessionLayout buffer) -> every raw field of `raw`
        (RawLayout's torch views of the byte buffer `buf`): one kernel launch and two small device copies (y | idx, user)."""
        from . import _lib_data
        from .ops import _p, _stream
        G, N = raw["counts"].shape[:2]
        _lib_data.launch("mobgt_sessions_to_raw", sdev.data_ptr() + slay.seq_off, sdev.data_ptr() + slay.len_off, _p(raw["counts"]),
                         _p(raw["x"]), _p(raw["time"]), _p(raw["cat"]), _p(raw["time_normal"]), _p(raw["n_nodes"]), _p(status),
                         G, Lp, N, _stream())
        buf[:slay.head_bytes].copy_(sdev[:slay.head_bytes], non_blocking=True)      # (y, idx: RawLayout's first two fields)
        raw["user"].view(-1).copy_(sdev[slay.user_off:slay.user_off + 4 * G].view(torch.int32), non_blocking=True)

    def __call__(self, sessions, idx0=0, n_pad=None):
        recs = [_as_record(s, f"session {i}") for i, s in enumerate(sessions) if s is not None]
        recs = [r for r in recs if r.n <= self.max_node]
        G = len(recs)
        if G == 0:
            raise ValueError("SessionCollator: no session to collate (none given, or every one longer than max_node)")
        n_max = max(r.n for r in recs)
        N = n_max if n_pad is None else int(n_pad)
        if N < n_max:
            raise ValueError(f"n_pad {N} is smaller than the longest trajectory ({n_max})")
        Lp = max(len(r.checkins) - 1 for r in recs)
        if not self.fits_kernel(Lp, N):
            return DeviceCollator.__call__(self, sessions_to_trajectories(recs), idx0, n_pad=n_pad)
        lay, slay = RawLayout(G, N), SessionLayout(G)
        host = np.zeros(slay.nbytes(Lp), dtype=np.uint8)
        self.pack_sessions(recs, idx0, slay.views_np(host, Lp))
        dev = torch.empty(lay.nbytes + host.size + 4 * G, dtype=torch.uint8, device=self.device)
        sdev = dev[lay.nbytes:lay.nbytes + host.size]
        sdev.copy_(torch.from_numpy(host), non_blocking=True)
        raw = lay.views_torch(dev)
        self.to_raw(sdev, slay, Lp, dev, raw, dev[lay.nbytes + host.size:].view(torch.int32))
        return self.finish(raw)

    # ---- the loops' hooks (DeviceCollator has the dict forms) ----------------------------------------------------------------
    def nodes_of(self, sample):
        return _as_record(sample).n

    @staticmethod
    def lengths_of(dataset):
        """A SessionDataset recorded every session's n when it validated them, a PrefixDataset every sample's; any other sequence
        of sessions is measured."""
        return [int(v) for v in dataset.n] if isinstance(dataset, (SessionDataset, PrefixDataset)) else [_as_record(s).n for s in dataset]

    def new_stage(self, lay, side, host=True):
        """DeviceCollator's stage, with the session bytes in place of its pinned raw arrays: a pinned SessionLayout buffer and
        its device twin, both grown to the longest history the bucket has seen.  The pinned raw buffer exists only once a
        batch of the bucket had to fall back to host conversion."""
        st = super().new_stage(lay, side, host=False)
        st.update(slay=SessionLayout(lay.G), spin=None, sdev=None, cap=0, Lp=0, mode=None,
                  raw_dev=st["dev_views"] if side else lay.views_torch(st["dev"]),
                  status=torch.zeros(lay.G, dtype=torch.int32, device=self.device))
        return st

    def stage_host(self, st, samples, idx0, N):
        recs = [_as_record(s) for s in samples]
        Lp = max(len(r.checkins) - 1 for r in recs)
        if not self.fits_kernel(Lp, N):
            if st["pin"] is None:
                self._host_stage(st)
            st["mode"] = "dicts"
            return self.pack_host(sessions_to_trajectories(recs), idx0=idx0, n_pad=N, out=st["np"])
        if Lp > st["cap"]:
            if st["sdev"] is not None:
                torch.cuda.synchronize(self.device)                   # (rare: nothing may still read the buffers that go)
            st["cap"] = max(64, 1 << (Lp - 1).bit_length())
            st["spin"] = torch.zeros(st["slay"].nbytes(st["cap"]), dtype=torch.uint8).pin_memory()
            # (not zeroed: upload copies every byte the kernel and the device copies read, and a fill queued here, on the
            #  current stream behind a running step, could land after the copy stream's upload and leave a batch of zeros)
            st["sdev"] = torch.empty(st["slay"].nbytes(st["cap"]), dtype=torch.uint8, device=self.device)
        st["mode"], st["Lp"] = "sessions", Lp
        return self.pack_sessions(recs, idx0, st["slay"].views_np(st["spin"].numpy(), Lp))

    def limit_violation(self, h, L):
        """DeviceCollator's checks, same order and same messages, on the packed sequences: x, user, y and the time slots from
        the check-ins; edge counts and degrees through bounds that cost nothing -- a count cannot exceed the largest
        multiplicity of a POI in the session, a degree cannot exceed n -- and exactly (session_graph, numpy) only for a
        session whose bound fails.  A session under the bound is under the limit, so the exact maximum over the failing
        ones is the batch's."""
        if "counts" in h:
            return super().limit_violation(h, L)
        bad = self._id_violation(h["seq"][:, :, 0], h, L)
        if bad:
            return bad
        recs = h["recs"]
        if "edge" in L:
            big = [r for r in recs if r.mult + 3 >= L["edge"]]
            if big:
                cmax = max(int(session_graph(r.checkins[:-1])["edge_type"].max()) for r in big)
                if cmax + 3 >= L["edge"]:
                    return "edge_input", cmax + 3, L["edge"]
        if "deg" in L:
            big = [r for r in recs if r.n + 1 >= L["deg"]]
            if big:
                nzs = [session_graph(r.checkins[:-1])["edge_type"] != 0 for r in big]
                dmax = max(max(int(z.sum(0).max()), int(z.sum(1).max())) for z in nzs)
                if dmax + 1 >= L["deg"]:
                    return "degree", dmax + 1, L["deg"]
        if "slots" in L:
            # (a node keeps the slot of its LAST visit: the largest slot of the history bounds the largest of the nodes)
            big = [r for r in recs if _slot_of(int(r.checkins[:-1, 1].max())) >= L["slots"]]
            if big:
                tmax = max(float(session_graph(r.checkins[:-1])["time_normal"].max()) for r in big)
                tmax = max(tmax, 0.0)                                 # (the padded batch's maximum includes the padding's 0)
                if int(tmax * 48) >= L["slots"]:
                    return "time_normal", tmax, L["slots"]
        return None

    def upload(self, st):
        if st["mode"] == "dicts":
            return super().upload(st)
        nb = st["slay"].nbytes(st["Lp"])
        st["sdev"][:nb].copy_(st["spin"][:nb], non_blocking=True)
        self.to_raw(st["sdev"], st["slay"], st["Lp"], st["dev"], st["raw_dev"], st["status"])


def _slot_of(t):
    """The time-slot index the model looks up for a raw slot value t: int(float32(t / 48) * 48), 0 for t = 0."""
    return int(float(np.float32(t / 48)) * 48) if t != 0 else 0


# ---- the POI table and the transition graphs from sessions (universe.py) ------------------------------------------------------------
from .universe import (BuiltUniverse, TransitionGraph, UniverseCounts, build_universe, first_seen_ids, universe_counts,  # noqa: E402,F401
                       universe_counts_host)


# ---- sessions from a raw check-in log (checkins.py) ---------------------------------------------------------------------------------
from .checkins import Sessionized, sessionize, sessionize_host  # noqa: E402,F401


# ---- every prefix of a session as a sample (prefixes.py) ----------------------------------------------------------------------------
from .prefixes import PrefixDataset, PrefixStats, prefix_stats, prefix_stats_host  # noqa: E402,F401


# ---- the Markov baseline on the same samples (baseline.py) --------------------------------------------------------------------------
from .baseline import MarkovBaseline  # noqa: E402,F401
from .prior import MarkovPrior  # noqa: E402,F401
from .geoprior import DistancePrior  # noqa: E402,F401
from .ctxprior import ContextPrior  # noqa: E402,F401
from .visitprior import VisitPrior  # noqa: E402,F401
