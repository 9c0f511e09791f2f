"""A fitted Markov baseline (baseline.MarkovBaseline) as a prior on a model's next-POI scores: log-counts of the baseline's three
tables, each with a weight, added to the [G, V] scores that Graphormer.metric_step / recommend_step rank -- on the device, in one
launch (csrc_prior/prior.hip through _prior), inside the loops' captured graphs.

Tables.  `mb.prior(user=wu, transition=wg, popularity=wp)` makes a MarkovPrior of a fitted MarkovBaseline.  It holds the
baseline's rowptr, col, ukey, U, P and three f32 tables as long as val, uval and pop:

    lg[e] = f32(log1p(val[e]))      lu[e] = f32(log1p(uval[e]))      lp[p] = f32(log1p(pop[p]))

All three are gathered from ONE table f32(np.log1p(np.arange(max_count + 1, dtype=float64))) made in numpy (log_table), on the
host and on the device alike, so both forms hold the same bits: no transcendental is evaluated in a kernel or in torch.  A count
is > 0 exactly where its logarithm is, which is what the rule tests.  The tables are counted over the TRAIN sessions only
(baseline.py): the prior sees nothing of a validation or test session.

Weights.  (wu, wg, wp) live in a device f32 [3] tensor the kernel reads, `prior.weights`; set_weights copies into it, so a
captured graph that blends stays valid when the weights change.  Only finite weights are taken.

Per row.  Row g of the scores belongs to a sample with the history ids hist[g, 0:n] (Restriction.hist(batch): the trajectory's
nodes, 0 = padding) and user[g] (batch.user = user + 1).
  * The anchor a is the LAST entry of hist[g] that is not 0 -- the anchor near="last" documents.  For graphs made from sessions
    (data.SessionCollator, sessions_to_trajectories) the nodes are ordered by their last visit, so it is the last history
    check-in; a hand-made dict stores distinct POIs in the order given, where its last node need not be the last check-in.  An
    id outside 1 .. P means no anchor.
  * u = user[g] - user_offset (1).  A user outside [0, U) has no user rows.
  * Column c is POI p = c + label_offset (model.label_offset).
  * Every operation is rounded to f32 on its own, no FMA, in exactly this order:

        s = scores[g, c]
        if 1 <= p <= P and pop(p) > 0:                      s = s + wp * lp[p - 1]
        if a exists and cg(a, p) > 0   (entry e of row a):   s = s + wg * lg[e]
        if additionally cu(u, a, p) > 0 (entry e'):           s = s + wu * lu[e']
        out[g, c] = s

    A term whose count is 0 is not added, so -0.0 survives where nothing applies; a term with weight 0 is added (x + 0.0: -0.0
    becomes +0.0, nothing else changes).  Non-finite scores go through the arithmetic as IEEE gives.  Entries of col whose
    column falls outside [0, V) are skipped silently: V and P need not agree (S-BIG has V = P + 1).
  * Tables that are not what fit makes: a rowptr pair that is descending or beyond nnz makes the row count as empty, an entry
    of col outside [0, P) is skipped, and both raise SBADINDEX in the status word.

`blend_host` is this rule in numpy f32 with plain loops over the entries of a row: the kernel's reference and the CPU form."""
import collections

import numpy as np
import torch

from . import _prior

WEIGHTS = ("user", "transition", "popularity")                          # the order of a weights row
MAX_SWEEP = 16                                                          # weight rows of one EvalLoop(prior_weights=)
SBADINDEX = _prior.SBADINDEX

PriorTables = collections.namedtuple("PriorTables", "rowptr col lg ukey lu lp U P")
PriorTables.__doc__ = "numpy: rowptr int64 [P + 1], col int32 [nnz], lg f32 [nnz], ukey int64 [nnzU], lu f32 [nnzU], lp f32 [P]; ints U, P"


def log_table(max_count):
    """f32(log1p(c)) for c in 0 .. max_count, computed in float64 and rounded once: what lg, lu and lp are gathered from."""
    return np.log1p(np.arange(int(max_count) + 1, dtype=np.float64)).astype(np.float32)


def check_weights(rows, what, names=WEIGHTS):
    """-> f32 numpy of the same shape; ValueError unless every value is finite (as f32 too).  names: what the weights are called."""
    try:
        w = np.asarray(rows, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: the weights must be numbers, got {rows!r}") from None
    with np.errstate(over="ignore"):
        w32 = w.astype(np.float32)
    if not np.isfinite(w32).all():
        raise ValueError(f"{what}: the weights ({', '.join(names)}) must be finite f32 values, got {w.tolist()}")
    return w32


def sweep_weights(W, what="prior_weights", names=WEIGHTS):
    """A weight sweep's rows -> f32 numpy [L, len(names)], 1 <= L <= MAX_SWEEP, finite; names: the columns, a prior's WEIGHTS
    (default MarkovPrior's: user, transition, popularity)."""
    w = np.asarray(W.detach().cpu().numpy() if isinstance(W, torch.Tensor) else W, dtype=np.float64)
    if w.ndim != 2 or w.shape[1] != len(names):
        raise ValueError(f"{what}: [L, {len(names)}] rows of ({', '.join(names)}) weights, got shape {tuple(w.shape)}")
    if not 1 <= w.shape[0] <= MAX_SWEEP:
        raise ValueError(f"{what}: {w.shape[0]} rows, one loop sweeps 1 .. {MAX_SWEEP} (MarkovPrior.tune splits a longer grid)")
    return check_weights(w, what, names)


def features_by_blend(prior, rows, label_offset, out, V=None, zeros=None):
    """What Prior.features does: `prior`'s blend of a zero buffer, once per weight of its own, with
    a unit weight row taken from a small identity kept on the prior's device -- plane k of out is then exactly the table value
    the rule adds for weight k, 0 where it adds nothing (a term with weight 0 adds +0.0).  out: f32 [n_weights, G, >= V] with
    unit column stride, its columns from V on left alone; V: the scored columns (default out.shape[2]); zeros: f32 [G, >= V]
    zeros to blend (default: allocated).  One launch per weight, no host read."""
    what = f"{type(prior).__name__}.features"
    n = prior.n_weights
    if not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.dim() != 3 or out.shape[0] != n or (out.shape[2] and out.stride(2) != 1):
        got = f"{out.dtype} {tuple(out.shape)}" if isinstance(out, torch.Tensor) else type(out).__name__
        raise ValueError(f"{what}: out must be f32 [{n}, G, >= V] with unit column stride, got {got}")
    G = out.shape[1]
    V = out.shape[2] if V is None else int(V)
    if not 0 <= V <= out.shape[2]:
        raise ValueError(f"{what}: V = {V} of {out.shape[2]} columns")
    if zeros is None:
        zeros = torch.zeros(G, V, dtype=torch.float32, device=out.device)
    elif zeros.dtype != torch.float32 or zeros.dim() != 2 or zeros.shape[0] != G or zeros.shape[1] < V:
        raise ValueError(f"{what}: zeros must be f32 [{G}, >= {V}], got {zeros.dtype} {tuple(zeros.shape)}")
    eye = getattr(prior, "_eye", None)
    if eye is None:
        eye = prior._eye = torch.eye(n, dtype=torch.float32, device=prior.device)
    for k in range(n):
        prior.blend(zeros[:, :V], rows, label_offset, out=out[k], weights=eye[k])
    return out


def blend_host(scores, hist, user, prior_tables, weights, label_offset, user_offset=1, status=None):
    """The rule of the module's docstring -> f32 numpy [G, V].  scores [G, V] f32; hist [G, n] integer ids; user [G] (or [G, 1]);
    prior_tables a PriorTables; weights (wu, wg, wp); status: a list or array whose [0] gets the SBADINDEX bit ORed in."""
    t = prior_tables
    s = np.array(scores, dtype=np.float32)
    G, V = s.shape
    hist, user = np.asarray(hist).reshape(G, -1), np.asarray(user).reshape(G)
    wu, wg, wp = (np.float32(w) for w in weights)
    P, lo, nnz = int(t.P), int(label_offset), len(t.col)
    # the popularity term: elementwise, a product rounded to f32 and then a sum rounded to f32
    c_lo, c_hi = max(0, 1 - lo), min(V, P + 1 - lo)                    # the columns whose POI is one of 1 .. P
    if c_hi > c_lo:
        lp = np.asarray(t.lp, dtype=np.float32)[c_lo + lo - 1:c_hi + lo - 1]
        term = (wp * lp).astype(np.float32)
        part = s[:, c_lo:c_hi]
        part[:, lp > 0] = (part[:, lp > 0] + term[lp > 0][None, :]).astype(np.float32)
    bad = 0
    for g in range(G):
        ids = hist[g][hist[g] != 0]
        a = int(ids[-1]) if len(ids) else 0
        if not 1 <= a <= P:
            continue
        r0, r1 = int(t.rowptr[a - 1]), int(t.rowptr[a])
        if r0 < 0 or r1 < r0 or r1 > nnz:
            bad |= SBADINDEX
            continue
        u = int(user[g]) - int(user_offset)
        mine = {}                                                      # cu(u, a, .): 0-based POI -> entry of ukey
        if 0 <= u < int(t.U) and len(t.ukey):
            base = (u * P + a - 1) * P
            i0, i1 = np.searchsorted(t.ukey, [base, base + P])
            mine = {int(k) - base: i for i, k in zip(range(int(i0), int(i1)), t.ukey[i0:i1])}
        for e in range(r0, r1):
            q = int(t.col[e])
            if q < 0 or q >= P:
                bad |= SBADINDEX
                continue
            c = q + 1 - lo
            if c < 0 or c >= V or not t.lg[e] > 0:
                continue
            v = np.float32(s[g, c] + np.float32(wg * np.float32(t.lg[e])))
            if q in mine and t.lu[mine[q]] > 0:
                v = np.float32(v + np.float32(wu * np.float32(t.lu[mine[q]])))
            s[g, c] = v
    if status is not None:
        status[0] |= bad
    return s


class Tuned:
    """tune and fit_weights of whatever has the priors' interface (WEIGHTS, n_weights, set_weights by name): what Prior and Stack
    share, so a bare prior and a stack are tuned and fitted by the same code.  NAME: what the messages call the class."""

    def tune(self, model, collator, val, grid, key="mrr", **loop_kw):
        """Evaluate every weights row of `grid` ([L, n_weights], columns WEIGHTS) on `val` with train.EvalLoop(model, collator, val,
        prior=self, prior_weights=..., **loop_kw) -- each batch is encoded once per loop, and a grid longer than MAX_SWEEP takes
        one loop per MAX_SWEEP rows -- then set the weights of the largest result[key] (the first of equal ones) and return the
        list of the L result dicts.  `val` must be held out of the sessions the tables were fitted on, and is not the test split:
        the weights are fitted to it."""
        from .train import EvalLoop
        what, n = f"{self.NAME}.tune", self.n_weights
        grid = np.asarray(grid, dtype=np.float64)
        if grid.ndim != 2 or grid.shape[1] != n or grid.shape[0] < 1:
            raise ValueError(f"{what}: grid must be [L >= 1, {n}] rows of ({', '.join(self.WEIGHTS)}) weights, got shape {tuple(grid.shape)}")
        check_weights(grid, what, self.WEIGHTS)
        results = []
        for i in range(0, len(grid), MAX_SWEEP):
            results += EvalLoop(model, collator, val, prior=self, prior_weights=grid[i:i + MAX_SWEEP], **loop_kw).run()
        best = max(range(len(results)), key=lambda i: (results[i][key], -i))
        self.set_weights(**dict(zip(self.WEIGHTS, grid[best].tolist())))
        return results

    def fit_weights(self, model, collator, val, l2=1e-3, tol=1e-7, max_passes=12, scale_model=True, **loop_kw):
        """Fit all n_weights weights at once by maximum likelihood of val's targets under softmax(blend) (priorfit.fit: Newton
        passes of train.PriorFitLoop(model, collator, val, self, **loop_kw), no grid), set them and return the priorfit.FitResult.
        `val` must be held out of the sessions the tables were fitted on, and is not the test split: the weights are fitted to it."""
        from .priorfit import fit
        return fit(self, model, collator, val, l2=l2, tol=tol, max_passes=max_passes, scale_model=scale_model, **loop_kw)


class Prior(Tuned):
    """What MarkovPrior, geoprior.DistancePrior, ctxprior.ContextPrior and visitprior.VisitPrior are: tables on one device, one weight per name of WEIGHTS
    and a status word, blended into [G, V] scores by one launch -- the interface the loops and Stack use of any prior.

    weights                f32 [n_weights] on the device, in WEIGHTS' order; written by set_weights only
    status                 int32 [1] on the device: kernels OR their S* bits into it and nothing clears it but reset_status (the
                           loops call it when a run starts and read the word once when it ends); check() reads it

    A subclass sets NAME, WEIGHTS, LIB (its ctypes module: MAX_G, I32, I64, launch), SKIPPED (what a status that is not zero
    means: the two halves of check's message) and HINTS (how for_loop's two refusals end), has `device` and `P` and a tables()
    that fills _host_tables, and gives blend its three own pieces: _rows, _blend_host and _launch."""

    n_weights = property(lambda self: len(self.WEIGHTS))

    def __init__(self, weights, status=None):
        self._host_weights = check_weights(weights, self.NAME, self.WEIGHTS).reshape(len(self.WEIGHTS))
        self.weights = torch.from_numpy(self._host_weights.copy()).to(self.device)
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device) if status is None else status
        self._host_tables = None

    def get_weights(self):
        """-> {name: weight} in WEIGHTS' order, as last set (the host's copy: no device read)."""
        return {k: float(v) for k, v in zip(self.WEIGHTS, self._host_weights)}

    def set_weights(self, *in_order, **by_name):
        """Copy new weights into the device tensor the kernel reads: positionally in WEIGHTS' order, or by name; None: that weight
        stays.  Non-finite: ValueError, and nothing is changed.  Graphs captured with this prior read the new values at their
        next replay."""
        what = f"{self.NAME}.set_weights"
        given = dict(zip(self.WEIGHTS, in_order))
        if len(in_order) > len(self.WEIGHTS) or not set(by_name) <= set(self.WEIGHTS) or set(by_name) & set(given):
            raise TypeError(f"{what}: the weights are ({', '.join(self.WEIGHTS)}), each given once; got {in_order!r} and {by_name!r}")
        given.update(by_name)
        new = [old if given.get(k) is None else given[k] for k, old in zip(self.WEIGHTS, self._host_weights.tolist())]
        self._host_weights = check_weights(new, what, self.WEIGHTS).reshape(len(self.WEIGHTS))
        self.weights.copy_(torch.from_numpy(self._host_weights.copy()), non_blocking=False)
        return self

    def reset_status(self):
        """Zero the status word on the current stream (what a loop does when a run starts)."""
        self.status.zero_()

    @classmethod
    def refuse(cls, bits, what):
        if bits:
            raise ValueError(f"{what}: the kernel skipped {cls.SKIPPED[0]} (status {bits}): {cls.SKIPPED[1]}")

    def check(self, what=None):
        """Read the status word (one host read); not zero: ValueError.  The word is left as it is."""
        self.refuse(int(self.status[0]), what or f"{self.NAME}.blend")

    def blend(self, scores, rows, label_offset, out=None, weights=None):
        """The blend of `scores` [G, V] f32 (rows of unit column stride) -> `out`; out=None: IN PLACE, and scores is returned.

        rows: what the subclass's _rows takes -- a collated batch, or the tensors themselves.  label_offset: model.label_offset,
        0 or 1.  out: f32 [G, >= V], scores itself or a buffer that does not overlap it; its columns from V on are left alone.
        weights: a device f32 [n_weights] view read in place of the prior's own (a row of a sweep).

        On the device ONE launch on the current stream: no allocation for a batch as the collators make it, no host read -- what
        the kernel flags lands in self.status (check()).  A CPU prior answers with its module's blend_host."""
        what = f"{self.NAME}.blend"
        if scores.dim() != 2 or scores.dtype != torch.float32 or (scores.shape[1] and scores.stride(1) != 1):
            raise ValueError(f"{what}: scores must be f32 [G, V] with unit column stride, got {scores.dtype} {tuple(scores.shape)}")
        G, V = scores.shape
        out = scores if out is None else out
        if out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != G or out.shape[1] < V or (out.shape[1] and out.stride(1) != 1):
            raise ValueError(f"{what}: out must be f32 [{G}, >= {V}] with unit column stride, got {out.dtype} {tuple(out.shape)}")
        if label_offset not in (0, 1):
            raise ValueError(f"{what}: label_offset must be 0 or 1 (model.label_offset), got {label_offset!r}")
        ids = self._rows(rows, G, what)                                 # ((name, tensor), ...), hist first
        w = self.weights if weights is None else weights
        if w.dtype != torch.float32 or w.numel() != self.n_weights or not w.is_contiguous():
            raise ValueError(f"{what}: weights must be a contiguous f32 [{self.n_weights}] view, got {w.dtype} {tuple(w.shape)}")
        for name, v in (("scores", scores), ("out", out), *ids, ("weights", w)):
            if v.device != self.device:
                raise ValueError(f"{what}: {name} is on {v.device}, the prior on {self.device}")
        ids = [v for _, v in ids]
        if self.device.type != "cuda":
            out[:, :V] = torch.from_numpy(self._blend_host(scores.numpy(), [v.numpy() for v in ids], w.tolist(), label_offset))
            return out
        if G > self.LIB.MAX_G:
            raise ValueError(f"{what}: {G} rows, one launch takes up to {self.LIB.MAX_G}")
        from .ops import _p, _stream
        ld = lambda v: v.stride(0) if G > 1 else max(V, v.stride(0))
        if out.data_ptr() == scores.data_ptr() and ld(out) != ld(scores):
            raise ValueError(f"{what}: out starts where scores starts with another row stride: in place means out is scores")
        code = lambda v: self.LIB.I64 if v.dtype == torch.int64 else self.LIB.I32
        hist, n = ids[0], ids[0].shape[1]
        with torch.cuda.device(self.device):                            # (what every *_blend_rows begins with, then the subclass's own)
            self._launch((_p(scores), ld(scores), _p(out), ld(out), G, V, int(label_offset), _p(hist), code(hist), max(hist.stride(0), n), n),
                         ids, w, _p, code, _stream())
        return out

    def for_loop(self, model, device, rows, what):
        """What a loop checks once, on the host, before it captures anything with this prior."""
        if torch.device(device) != self.device:
            raise ValueError(f"{what}: the prior is on {self.device}, the loop on {torch.device(device)}: {self.HINTS[0]}")
        V, lo = model.out_proj.out_features, model.label_offset
        if self.P > V - 1 + lo:
            raise ValueError(f"{what}: the prior has POIs 1 .. {self.P}, the model scores {V} columns for POIs {lo} .. {V - 1 + lo}: "
                             f"{self.HINTS[1]}")
        if rows > self.LIB.MAX_G:
            raise ValueError(f"{what}: batch_size {rows}, one blend launch takes up to {self.LIB.MAX_G} rows")

    def features(self, rows, label_offset, out, V=None, zeros=None):
        """out[k, g, c] = what the rule adds to scores[g, c] per unit of weight k (WEIGHTS' order; 0 where it adds nothing): one
        blend of zeros per weight (features_by_blend).  out: f32 [n_weights, G, >= V]; rows, label_offset as blend's."""
        return features_by_blend(self, rows, label_offset, out, V, zeros)


class MarkovPrior(Prior):
    """The tables of the module's docstring on one device, their weights (user, transition, popularity) and a status word (Prior).

    P, U                   as the baseline's
    rowptr, col, ukey      the baseline's own tensors (shared, not copied)
    lg, lu, lp             f32 [nnz], [nnzU], [P]

    rows of blend: a collated batch (hist = Restriction.hist(batch), user = batch.user) or a (hist [G, n], user [G]) pair of
    int32 / int64 tensors.  The launch is mobgt_prior_blend_rows; it ORs SBADINDEX into status, and so does a CPU prior's blend."""

    NAME, WEIGHTS, LIB = "MarkovPrior", WEIGHTS, _prior
    SKIPPED = ("table rows or entries", "a rowptr pair was descending or beyond nnz, or an entry of col was outside [0, P) -- the "
               "tables are not what MarkovBaseline.fit makes")
    HINTS = ("fit the baseline on the loop's device (MarkovBaseline.fit(..., device=...))",
             "the baseline was not fitted on the model's universe")

    def __init__(self, P, U, rowptr, col, lg, ukey, lu, lp, weights):
        self.P, self.U, self.rowptr, self.col, self.lg, self.ukey, self.lu, self.lp = int(P), int(U), rowptr, col, lg, ukey, lu, lp
        super().__init__(weights)

    @property
    def device(self):
        return self.lp.device

    @classmethod
    def from_baseline(cls, mb, user=1.0, transition=1.0, popularity=1.0):
        """One log_table for the largest count of the three tables, uploaded once; lg, lu and lp are gathers from it."""
        weights = check_weights([user, transition, popularity], "MarkovBaseline.prior")
        g = mb.graph
        top = max([int(v.max()) for v in (g.val, mb.uval, mb.pop) if v.numel()] + [0])
        table = torch.from_numpy(log_table(top)).to(mb.device)
        lg, lu, lp = (table[v.long()] for v in (g.val, mb.uval, mb.pop))
        return cls(mb.P, mb.U, g.rowptr, g.col, lg, mb.ukey, lu, lp, weights)

    def tables(self):
        """-> PriorTables: the tables as numpy arrays (one download, kept), what blend_host takes."""
        if self._host_tables is None:
            n = lambda v: v.detach().cpu().numpy()
            self._host_tables = PriorTables(n(self.rowptr), n(self.col), n(self.lg), n(self.ukey), n(self.lu), n(self.lp), self.U, self.P)
        return self._host_tables

    @staticmethod
    def _rows(rows, G, what):
        hist, user = rows if isinstance(rows, (tuple, list)) else (rows.x.reshape(rows.x.shape[0], -1), rows.user)
        hist, user = hist.reshape(hist.shape[0], -1), user.reshape(-1)
        if hist.shape[0] != G or user.shape[0] != G:
            raise ValueError(f"{what}: {G} rows of scores, {hist.shape[0]} of hist and {user.shape[0]} users")
        for name, v in (("hist", hist), ("user", user)):
            if v.dtype not in (torch.int32, torch.int64):
                raise TypeError(f"{what}: {name} must be int32 or int64 ids, got {v.dtype}")
        if hist.shape[1] and hist.stride(1) != 1:
            hist = hist.contiguous()
        return ("hist", hist), ("user", user)

    def _blend_host(self, scores, ids, w, label_offset):
        status = [0]
        res = blend_host(scores, *ids, self.tables(), w, label_offset, status=status)
        self.status |= status[0]
        return res

    def _launch(self, head, ids, w, _p, code, stream):
        user = ids[1]
        _prior.launch("mobgt_prior_blend_rows", *head, _p(user), code(user), max(user.stride(0), 1), 1,
                      _p(self.rowptr), _p(self.col), _p(self.lg), int(self.col.numel()),
                      _p(self.ukey), _p(self.lu), int(self.ukey.numel()), self.U, _p(self.lp), self.P, _p(w), _p(self.status), stream)


class Stack(Tuned):
    """One or more priors blended in the order given, behind the interface the loops use of any prior (EvalLoop / PredictLoop,
    Graphormer.metric_step / recommend_step): prior.Stack(mb.prior(), mb.distance_prior(pair_bins)).

    priors      the members, a tuple: any Prior (MarkovPrior, geoprior.DistancePrior, ctxprior.ContextPrior, visitprior.VisitPrior), or anything with their
                interface
    WEIGHTS     the members' names concatenated, e.g. ("user", "transition", "popularity", "distance"); no name twice
    n_weights   len(WEIGHTS): the width of a weights row (blend(weights=), EvalLoop(prior_weights=), tune's grid)

    Each member keeps its own device weights and status word; a blend is one launch per member: the first writes `out`, the rest
    run in place on it, so the result is the members' rules applied in turn, bit for bit.  tune and fit_weights are the bare
    priors' own (Tuned); a Stack is no Prior, because it has no weights tensor of its own."""

    NAME = "prior.Stack"

    def __init__(self, *priors):
        if not priors:
            raise ValueError("prior.Stack: at least one prior")
        for p in priors:
            missing = [a for a in ("WEIGHTS", "n_weights", "blend", "for_loop", "check", "reset_status", "set_weights", "get_weights")
                       if not hasattr(p, a)]
            if missing:
                raise TypeError(f"prior.Stack: {type(p).__name__} is no prior (it has no {', '.join(missing)})")
        self.priors = tuple(priors)
        self.WEIGHTS = tuple(n for p in priors for n in p.WEIGHTS)
        self.n_weights = len(self.WEIGHTS)
        twice = list(dict.fromkeys(n for n in self.WEIGHTS if self.WEIGHTS.count(n) > 1))
        if twice:
            raise ValueError(f"prior.Stack: the weights {', '.join(twice)} belong to more than one member: set_weights could not tell them apart")
        devices = {str(p.device) for p in priors}
        if len(devices) > 1:
            raise ValueError(f"prior.Stack: the members are on {', '.join(sorted(devices))}: fit them on one device")

    @property
    def device(self):
        return self.priors[0].device

    def _split(self, weights, what):
        """A contiguous f32 [n_weights] view -> one view per member (None: every member reads its own)."""
        if weights is None:
            return [None] * len(self.priors)
        if not isinstance(weights, torch.Tensor) or weights.dtype != torch.float32 or weights.numel() != self.n_weights or not weights.is_contiguous():
            got = f"{weights.dtype} {tuple(weights.shape)}" if isinstance(weights, torch.Tensor) else type(weights).__name__
            raise ValueError(f"{what}: weights must be a contiguous f32 [{self.n_weights}] view ({', '.join(self.WEIGHTS)}), got {got}")
        flat, out, at = weights.reshape(-1), [], 0
        for p in self.priors:
            out.append(flat[at:at + p.n_weights])
            at += p.n_weights
        return out

    def blend(self, scores, rows, label_offset, out=None, weights=None):
        """The members' blends in turn: the first from `scores` into `out` (out=None: in place, and scores is returned), the
        others in place on the V columns it wrote.  weights: a device f32 [n_weights] view, split per member in order."""
        views = self._split(weights, "prior.Stack.blend")
        res = self.priors[0].blend(scores, rows, label_offset, out=out, weights=views[0])
        into = res[:, :scores.shape[1]]
        for p, w in zip(self.priors[1:], views[1:]):
            p.blend(into, rows, label_offset, weights=w)
        return res

    def for_loop(self, model, device, rows, what):
        for p in self.priors:
            p.for_loop(model, device, rows, what)

    def reset_status(self):
        for p in self.priors:
            p.reset_status()

    def check(self, what="prior.Stack.blend"):
        for p in self.priors:
            p.check(what)

    def get_weights(self):
        """-> {name: weight} of every member, in WEIGHTS' order (the hosts' copies: no device read)."""
        return {k: v for p in self.priors for k, v in p.get_weights().items()}

    def set_weights(self, **by_name):
        """set_weights of the members that own the names given; an unknown name or a non-finite value: ValueError, and nothing
        is changed."""
        unknown = [k for k in by_name if k not in self.WEIGHTS]
        if unknown:
            raise ValueError(f"prior.Stack.set_weights: no weight called {', '.join(unknown)} (the stack has {', '.join(self.WEIGHTS)})")
        check_weights([v for v in by_name.values() if v is not None], "prior.Stack.set_weights", tuple(k for k, v in by_name.items() if v is not None))
        for p in self.priors:
            mine = {k: v for k, v in by_name.items() if k in p.WEIGHTS}
            if mine:
                p.set_weights(**mine)
        return self

    def features(self, rows, label_offset, out, V=None, zeros=None):
        """The members' features in WEIGHTS' order: member i fills its n_weights planes of out, f32 [n_weights, G, >= V]."""
        if not isinstance(out, torch.Tensor) or out.dim() != 3 or out.shape[0] != self.n_weights:
            got = tuple(out.shape) if isinstance(out, torch.Tensor) else type(out).__name__
            raise ValueError(f"prior.Stack.features: out must be f32 [{self.n_weights}, G, >= V], got {got}")
        at = 0
        for p in self.priors:
            p.features(rows, label_offset, out[at:at + p.n_weights], V, zeros)
            at += p.n_weights
        return out
