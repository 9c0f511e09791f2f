"""What an evaluation or a recommendation is restricted to, decided once per loop or per call and handed to
`Graphormer.metric_step` / `recommend_step` as one object: leave out the trajectory's own POIs, a candidate set shared by the
rows, the rows' own candidates within a radius, the split by revisits -- and the label offset all of them are stated in."""
import torch

from . import ops


class Restriction:
    """exclude_visited, split_revisits: flags.  allow: ops.pack_allow words shared by the rows, or None.  near: (pos,
    chord2_max, mode, words) -- ops.pack_positions' table, ops.chord2_of_km(r), "last" / "any" and an int32
    [>= G, >= ceil(V / 32)] device buffer the rows' words are written into -- or None.  label_offset: an id p of y or x is
    column p - label_offset of the scores (model.label_offset).  Building one allocates nothing."""

    def __init__(self, label_offset, exclude_visited=False, allow=None, split_revisits=False, near=None):
        self.label_offset = int(label_offset)
        self.exclude_visited, self.split_revisits = bool(exclude_visited), bool(split_revisits)
        self.allow, self.near = allow, near

    @staticmethod
    def radius(collator, within_km, coords, near):
        """A loop's within_km= / coords= / near= checked on the host, before anything is allocated:
        None, or (coordinate table, whether it is in radians, chord2_max, mode)."""
        ops.near_mode(near)                                               # (a bad mode string is refused here, on the host)
        if within_km is None:
            return None
        chord2_max = ops.chord2_of_km(within_km)
        if coords is not None:
            return torch.as_tensor(coords), False, chord2_max, near
        if getattr(collator, "coords", None) is None:
            raise ValueError("within_km: no POI coordinates -- pass coords=[P + 1, 2] lat / lon in degrees (row 0 the pad POI), or "
                             "use a collator built with coords=")
        return collator.coords, True, chord2_max, near                    # (DeviceCollator keeps radians)

    @classmethod
    def on_device(cls, label_offset, V, rows, device, exclude_visited=False, candidates=None, split_revisits=False, radius=None):
        """A loop's restriction for `rows` rows of V scores: candidates (POI ids in y's label space) packed into allow words,
        `radius` (Restriction.radius' result) into positions and one [rows, W] words buffer -- once, so that the loop's graphs
        read and write them at fixed addresses."""
        allow = near = None
        if candidates is not None:
            allow = ops.pack_allow(torch.as_tensor(candidates).to(device), V, label_offset)
        if radius is not None:
            table, radians, chord2_max, mode = radius
            near = (ops.pack_positions(table.to(device), V, label_offset, radians=radians), chord2_max, mode,
                    torch.zeros(rows, (V + 31) // 32, dtype=torch.int32, device=device))
        return cls(label_offset, exclude_visited, allow, split_revisits, near)

    @property
    def active(self):
        return self.exclude_visited or self.split_revisits or self.allow is not None or self.near is not None

    @staticmethod
    def hist(batch):
        """[G, n]: the trajectories' POI ids (x holds them in y's label space, 0 = padding)"""
        return batch.x.reshape(batch.x.shape[0], -1)

    def allow_for(self, hist):
        """The `allow` of ops.topk_rows / ops.rank_metrics_masked for these rows: with a radius their own words (ops.near_words
        on hist, the shared words ANDed in, written into the buffer -- inside a captured graph when the step is captured), else
        the shared words"""
        if self.near is None:
            return self.allow
        pos, chord2_max, mode, words = self.near
        return ops.near_words(pos, hist, self.label_offset, chord2_max, mode, allow=self.allow, out=words[:hist.shape[0]])

    def exclude(self, hist):
        return hist if self.exclude_visited else None
