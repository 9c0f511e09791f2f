"""Check-in sessions from a raw check-in log: the last input that came from the reference's offline Python run
(graphormer/foursquare_process.py: load_trajectory_from_tweets and filter_users_by_length :115-260, build_users_locations_dict
:262-294, prepare_neural_data :377-482).

A log is N records in log order: `user`, `poi`, `cat` (any ids) and `t`, int64 seconds of the LOCAL wall clock (calendar.timegm of
the local time string the reference builds at :132-134; the reference's own number depends on the machine's time zone through
mktime / localtime), optionally `lat` and `lon`.  The rule (golden G14 pins it to the reference's own run):

1.  Count records per user and per POI over the whole log.  A user is kept with >= trace_min records, a POI with >=
    global_visit.  Users are ordered by count descending, ties by first appearance in the log (:185).
2.  The cut, per user, over the user's records in log order (the log is not sorted by time, a negative gap is legal).  A record
    whose POI is not kept is skipped and changes no state (:211-214).  For each remaining record g = t - t_prev, t_prev the
    user's previous remaining record whether or not it entered a session (:246), and s = the length of the user's current
    session.  The first remaining record starts a session; else g >= 3600 hour_gap or s > session_max starts one; else
    g >= 60 min_gap appends; else the record is dropped (:230-243).  The fullness test comes first: a record 1 s after a full
    session starts a new one, and a session reaches at most session_max + 1 records.
3.  Sessions of >= session_min records are kept and renumbered, users with >= sessions_min kept sessions survive (:249-259) and
    are numbered 0 .. U - 1 in the order of step 1.
4.  The output check-ins go users in that order, sessions in order, records in order.  POIs are numbered 1 .. P by first
    appearance in this output (:276-283), categories 1 .. n_cat by first appearance of the check-ins' own categories (:284-289); a
    row carries the first-seen category of its POI, not its own (:293-294, :425).  The slot is (t mod 86400) div 1800 with a
    floor mod (tid_list_1day48).  A POI's coordinates are those of its first output check-in (:279).
5.  Per user, split = int(np.floor(train_split * n_sessions)) in float64; the first `split` sessions are train (:433-435).  A
    surviving user with split == 0 crashes the reference at :477 and is a ValueError naming the user here.

`sessionize` runs it on the device (csrc_checkins/sessions.hip through _checkins; torch.sort and torch.cumsum between the
launches); `sessionize_host` is the same rule as a plain loop: the CPU form and the kernels' reference."""
import dataclasses

import numpy as np
import torch

from .universe import first_seen_ids

DEFAULTS = dict(trace_min=10, global_visit=10, hour_gap=24, min_gap=10, session_min=5, session_max=10, sessions_min=2, train_split=0.8)
DEVICE_SESSION_MAX = 15                            # (= _checkins.MAX_SESSION_MAX: a map of the session length in one 64-bit word)


@dataclasses.dataclass
class Sessionized:
    """What `sessionize` / `sessionize_host` return; numpy on the host.  S sessions, M output check-ins, U users, P POIs."""
    dataset: object                # data.SessionDataset: seq [M, 3] (poi, slot, category), offsets [S + 1], users [S], n, mult
    train: np.ndarray              # bool [S]
    user_ids: np.ndarray           # [U]: the raw id of new user id k
    poi_ids: np.ndarray            # [P]: the raw id of new POI id k + 1
    cat_ids: np.ndarray            # [n_cat]: the raw id of new category id k + 1
    coords_deg: object             # float64 [P, 2] lat, lon of every POI's first output check-in, or None
    kept: np.ndarray               # int64 [M]: the log position of every output check-in
    users_order: np.ndarray        # the raw ids of the users kept by trace_min, in the order of step 1 (survivors or not)


def _prepare(user, poi, cat, t, lat, lon, dense, p, device_form):
    """Every ValueError, before anything is launched or looped over -> (user, poi, cat int32 dense ids; t int64; lat, lon float64
    or None; (U0, P0, C0); the three lookups raw id of dense id; the parameters as a dict)."""
    unknown = set(p) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"sessionize: unknown parameter(s) {sorted(unknown)}")
    p = dict(DEFAULTS, **p)
    cols = dict(user=user, poi=poi, cat=cat, t=t)
    if (lat is None) != (lon is None):
        raise ValueError("sessionize: lat and lon come together")
    if lat is not None:
        cols.update(lat=lat, lon=lon)
    cols = {k: v if isinstance(v, np.ndarray) else np.asarray(list(v)) for k, v in cols.items()}
    N = len(cols["t"])
    for k, v in cols.items():
        if v.ndim != 1 or len(v) != N:
            raise ValueError(f"sessionize: {k} has shape {v.shape}, t has {N} records: one flat array per column, of equal length")
    if N >= 2 ** 31:
        raise ValueError(f"sessionize: {N} records, the kernels index records with 31 bits (N < 2**31): cut the log by users")
    tt = cols["t"]
    if N and not np.issubdtype(tt.dtype, np.integer):
        raise ValueError(f"sessionize: t must be integer seconds of the local wall clock, got {tt.dtype}")
    for k in ("trace_min", "global_visit", "hour_gap", "min_gap", "session_min", "session_max", "sessions_min"):
        if not isinstance(p[k], (int, np.integer)) or isinstance(p[k], bool):
            raise ValueError(f"sessionize: {k} must be an integer, got {p[k]!r}")
        if p[k] < 0:
            raise ValueError(f"sessionize: {k} = {p[k]} is negative")
        p[k] = int(p[k])
    if p["session_min"] < 2:
        raise ValueError(f"sessionize: session_min = {p['session_min']}, a session needs a history and a target (session_min >= 2)")
    top = DEVICE_SESSION_MAX if device_form else 2 ** 31 - 2
    if not 1 <= p["session_max"] <= top:
        raise ValueError(f"sessionize: session_max = {p['session_max']} is not in 1 .. {top}"
                         + (" (the device form keeps the session length in 4 bits; sessionize_host takes more)" if device_form else ""))
    p["train_split"] = float(p["train_split"])
    if not 0.0 < p["train_split"] <= 1.0:
        raise ValueError(f"sessionize: train_split = {p['train_split']} is not in (0, 1]")
    if p["hour_gap"] * 3600 >= 2 ** 62 or p["min_gap"] * 60 >= 2 ** 62:
        raise ValueError("sessionize: a gap threshold does not fit 62 bits of seconds")
    ids, lookups, sizes = [], [], []
    if dense is not None:
        if len(dense) != 3 or any(int(d) < 1 or int(d) >= 2 ** 28 for d in dense):
            raise ValueError(f"sessionize: dense = (U0, P0, C0), each in 1 .. 2**28 - 1, got {dense!r}")
        for k, size in zip(("user", "poi", "cat"), dense):
            v = cols[k]
            if N and not np.issubdtype(v.dtype, np.integer):
                raise ValueError(f"sessionize: with dense=, {k} must hold integer ids, got {v.dtype}")
            if N and (v.min() < np.iinfo(np.int32).min or v.max() > np.iinfo(np.int32).max):
                raise ValueError(f"sessionize: a {k} id does not fit int32")
            ids.append(np.ascontiguousarray(v, dtype=np.int32))
            lookups.append(np.arange(1, int(size) + 1, dtype=np.int64))
            sizes.append(int(size))
    else:
        for k in ("user", "poi", "cat"):
            d, lookup = first_seen_ids(cols[k]) if N else (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
            ids.append(np.ascontiguousarray(d, dtype=np.int32))
            lookups.append(lookup)
            sizes.append(max(len(lookup), 1))
        if max(sizes) >= 2 ** 28:
            raise ValueError("sessionize: more than 2**28 - 1 distinct ids in a column")
    f64 = lambda v: None if v is None else np.ascontiguousarray(v, dtype=np.float64)
    return (ids[0], ids[1], ids[2], np.ascontiguousarray(tt, dtype=np.int64), f64(cols.get("lat")), f64(cols.get("lon")), tuple(sizes),
            lookups, p)


def _bad_ids(user, poi, cat, sizes):
    """The records with an id outside its range, and the ValueError that names the first."""
    bad = np.zeros(len(user), dtype=bool)
    for v, size in zip((user, poi, cat), sizes):
        bad |= (v < 1) | (v > size)
    return bad


def _id_error(user, poi, cat, sizes, where):
    bad = _bad_ids(user, poi, cat, sizes)
    i = int(np.argmax(bad)) if bad.any() else -1
    detail = f": record {i} has (user, poi, cat) = ({int(user[i])}, {int(poi[i])}, {int(cat[i])})" if i >= 0 else ""
    return ValueError(f"sessionize: {where} an id outside 1 .. U0 / 1 .. P0 / 1 .. C0 = {sizes}{detail}")


def _zero_split(raw_user, n_sessions, train_split):
    raw_user = raw_user.item() if isinstance(raw_user, np.generic) else raw_user
    return ValueError(f"sessionize: user {raw_user!r} survives with {n_sessions} session(s), of which floor({train_split} * "
                      f"{n_sessions}) = 0 are train: the reference crashes here (foursquare_process.py:477); raise sessions_min or "
                      "train_split")


def _result(seq, offsets, users, n, mult, train, kept, user_dense, order_dense, lookups, poi_log, cat_log, lat, lon, poi, cat):
    """The common end of both forms: the packed arrays and log positions -> Sessionized."""
    from .data import SessionDataset
    ds = SessionDataset.from_packed(seq, offsets, users, n, mult)
    poi_log, cat_log = np.asarray(poi_log, dtype=np.int64), np.asarray(cat_log, dtype=np.int64)
    coords = None if lat is None else np.stack([lat[poi_log], lon[poi_log]], 1).reshape(-1, 2)
    take = lambda lookup, dense: lookup[np.asarray(dense, dtype=np.int64) - 1] if len(dense) else lookup[:0]
    return Sessionized(ds, np.asarray(train, dtype=bool), take(lookups[0], user_dense), take(lookups[1], poi[poi_log]),
                       take(lookups[2], cat[cat_log]), coords, np.asarray(kept, dtype=np.int64), take(lookups[0], order_dense))


# ---- the host form ----------------------------------------------------------------------------------------------------------------
def sessionize_host(user, poi, cat, t, lat=None, lon=None, *, dense=None, **params):
    """The rule of the module's docstring as a plain loop over the records -> Sessionized.  `dense=(U0, P0, C0)`: the ids are
    already integers in 1 .. U0 / 1 .. P0 / 1 .. C0 and are taken as they are (an id outside its range is a ValueError);
    otherwise raw ids of any hashable kind are numbered with first_seen_ids."""
    user, poi, cat, t, lat, lon, sizes, lookups, p = _prepare(user, poi, cat, t, lat, lon, dense, params, device_form=False)
    if _bad_ids(user, poi, cat, sizes).any():
        raise _id_error(user, poi, cat, sizes, "the log holds")
    N = len(t)
    records, venues = {}, {}                                           # (dicts keep insertion order: first appearance)
    for i in range(N):
        records.setdefault(int(user[i]), []).append(i)
        venues[int(poi[i])] = venues.get(int(poi[i]), 0) + 1
    order = sorted((u for u in records if len(records[u]) >= p["trace_min"]), key=lambda u: -len(records[u]))      # (stable)
    hour_s, min_s = 3600 * p["hour_gap"], 60 * p["min_gap"]
    survivors = []                                                     # (dense user, its kept sessions as lists of log positions)
    for u in order:
        sessions, last = [], None
        for i in records[u]:
            if venues[int(poi[i])] < p["global_visit"]:
                continue
            ti = int(t[i])
            if last is None:
                sessions.append([i])
            else:
                g = ti - last
                if g >= hour_s or len(sessions[-1]) > p["session_max"]:
                    sessions.append([i])
                elif g >= min_s:
                    sessions[-1].append(i)
            last = ti
        keep = [s for s in sessions if len(s) >= p["session_min"]]
        if keep and len(keep) >= p["sessions_min"]:
            survivors.append((u, keep))
    vid, cid, poi_log, cat_log, first_cat = {}, {}, [], [], {}
    rows, offsets, users, train, kept = [], [0], [], [], []
    for un, (u, keep) in enumerate(survivors):
        split = int(np.floor(p["train_split"] * len(keep)))
        if split == 0:
            raise _zero_split(lookups[0][u - 1], len(keep), p["train_split"])
        for k, s in enumerate(keep):
            for i in s:
                pi, ci = int(poi[i]), int(cat[i])
                if pi not in vid:
                    vid[pi] = len(vid) + 1
                    first_cat[pi] = ci
                    poi_log.append(i)
                if ci not in cid:
                    cid[ci] = len(cid) + 1
                    cat_log.append(i)
                kept.append(i)
            offsets.append(len(kept))
            users.append(un)
            train.append(k < split)
    for i in kept:
        pi = int(poi[i])
        rows.append((vid[pi], (int(t[i]) % 86400) // 1800, cid[first_cat[pi]]))
    seq = np.asarray(rows, dtype=np.int32).reshape(-1, 3)
    n, mult = [], []
    for a, b in zip(offsets[:-1], offsets[1:]):
        _, cnt = np.unique(seq[a:b - 1, 0], return_counts=True)
        n.append(len(cnt))
        mult.append(int(cnt.max()))
    return _result(seq, np.asarray(offsets, dtype=np.int64), np.asarray(users, dtype=np.int64), np.asarray(n, dtype=np.int32),
                   np.asarray(mult, dtype=np.int32), train, kept, [u for u, _ in survivors], order, lookups, poi_log, cat_log, lat, lon,
                   poi, cat)


# ---- the device path --------------------------------------------------------------------------------------------------------------
def sessionize(user, poi, cat, t, lat=None, lon=None, *, dense=None, device="cuda", **params):
    """sessionize_host on the device -> the same Sessionized, integer for integer.  Everything about the arguments is validated
    on the host before anything is launched.  With `dense=(U0, P0, C0)` the int32 ids go to the device as they are: an id
    outside its range is never used as an index, its record is skipped by the kernels and reported through their status word,
    which is a ValueError here.  Without a GPU (`device="cpu"`) this is sessionize_host.

    Launches: mobgt_checkins_count, torch.sort (users), mobgt_checkins_keys, torch.sort (records), mobgt_checkins_cut,
    torch.cumsum, mobgt_checkins_sessions, five torch.cumsum, mobgt_checkins_first, two torch.cumsum, mobgt_checkins_emit."""
    device = torch.device(device)
    if device.type != "cuda":
        return sessionize_host(user, poi, cat, t, lat, lon, dense=dense, **params)
    user, poi, cat, t, lat, lon, sizes, lookups, p = _prepare(user, poi, cat, t, lat, lon, dense, params, device_form=True)
    from . import _checkins as ck
    from .ops import _p, _stream
    N, (U0, P0, C0) = len(t), sizes
    with torch.cuda.device(device):
        up = lambda a: torch.from_numpy(a).to(device)
        i32 = lambda n: torch.empty(int(n), dtype=torch.int32, device=device)
        i64 = lambda n: torch.empty(int(n), dtype=torch.int64, device=device)
        cum = lambda v: torch.cumsum(v, 0, dtype=torch.int64)
        last = lambda *cs: [int(v) for v in torch.stack([c[-1] if c.numel() else c.new_zeros(()) for c in cs]).cpu()]
        d_user, d_poi, d_cat, d_t = up(user), up(poi), up(cat), up(t)
        ucnt, pcnt, ufirst, ukey, status = i32(U0), i32(P0), i32(U0), i64(U0), i32(1)
        ck.launch("mobgt_checkins_count", _p(d_user), _p(d_poi), _p(d_cat), N, U0, P0, C0, p["trace_min"], _p(ucnt), _p(pcnt),
                  _p(ufirst), _p(ukey), _p(status), _stream())
        ukey, uorder = torch.sort(ukey)
        U1 = int(torch.searchsorted(ukey, torch.tensor([ck.NOKEY], dtype=torch.int64, device=device))[0])
        bits = int(status[0])
        if bits:
            raise _id_error(user, poi, cat, sizes, f"the kernel skipped records (status {bits}) with")
        urank = torch.full((U0,), -1, dtype=torch.int32, device=device)
        urank[uorder[:U1]] = torch.arange(U1, dtype=torch.int32, device=device)
        keys = i64(N)
        ck.launch("mobgt_checkins_keys", _p(d_user), _p(d_poi), _p(d_cat), N, U0, P0, C0, _p(urank), U1, _p(pcnt), p["global_visit"],
                  _p(keys), _stream())
        keys = torch.sort(keys).values
        R = int(torch.searchsorted(keys, torch.tensor([ck.NOKEY], dtype=torch.int64, device=device))[0]) if N else 0
        keys = keys[:R].contiguous()
        start, member = i32(R), i32(R)
        ck.launch("mobgt_checkins_cut", _p(keys), R, _p(d_t), N, U1, 3600 * p["hour_gap"], 60 * p["min_gap"], p["session_max"],
                  _p(start), _p(member), _p(status), _stream())
        scum = cum(start)
        S0, = last(scum)
        slen, suser, sfinal, outlen = i32(S0), i32(S0), i32(S0), i32(S0)
        ukept, usurv, ukept_s, split, emit = i32(U1), i32(U1), i32(U1), i32(U1), i32(R)
        ck.launch("mobgt_checkins_sessions", _p(keys), _p(start), _p(member), _p(scum), R, S0, U1, p["session_min"], p["sessions_min"],
                  p["train_split"], _p(slen), _p(suser), _p(ukept), _p(sfinal), _p(outlen), _p(usurv), _p(ukept_s), _p(split),
                  _p(emit), _p(status), _stream())
        scum2, lcum, ucum, kcum, ocum = cum(sfinal), cum(outlen), cum(usurv), cum(ukept_s), cum(emit)
        S, M, U, S_users, M_records, bits = last(scum2, lcum, ucum, kcum, ocum, status.long())
        order_dense = (uorder[:U1] + 1).cpu().numpy()
        if bits & ck.SZEROSPLIT:
            k, sp, surv = ukept.cpu().numpy(), split.cpu().numpy(), usurv.cpu().numpy().astype(bool)
            r = int(np.argmax(surv & (sp < 1)))
            raise _zero_split(lookups[0][order_dense[r] - 1], int(k[r]), p["train_split"])
        if bits or S_users != S or M_records != M:
            raise RuntimeError(f"sessionize: the kernels disagree with themselves (status {bits}, sessions {S} / {S_users}, check-ins "
                               f"{M} / {M_records})")
        kept, pfirst, cfirst, pflag, cflag = i64(M), i32(P0), i32(C0), i32(M), i32(M)
        ck.launch("mobgt_checkins_first", _p(keys), _p(emit), _p(ocum), R, M, _p(d_poi), _p(d_cat), N, P0, C0, _p(kept), _p(pfirst),
                  _p(cfirst), _p(pflag), _p(cflag), _p(status), _stream())
        pnum, cnum = cum(pflag), cum(cflag)
        P, n_cat = last(pnum, cnum)
        seq, poi_log, cat_log = torch.empty(M, 3, dtype=torch.int32, device=device), i32(P), i32(n_cat)
        offsets, users_new, train = i64(S + 1), i64(S), torch.empty(S, dtype=torch.uint8, device=device)
        n, mult, user_log = i32(S), i32(S), i32(U)
        ck.launch("mobgt_checkins_emit", _p(kept), _p(pflag), _p(cflag), _p(pnum), _p(cnum), M, _p(pfirst), _p(cfirst), _p(d_poi),
                  _p(d_cat), _p(d_t), N, P0, C0, P, n_cat, _p(sfinal), _p(suser), _p(scum2), _p(lcum), S0, S, _p(ucum), _p(kcum),
                  _p(ukept_s), _p(split), U1, U, _p(seq), _p(poi_log), _p(cat_log), _p(offsets), _p(users_new), _p(train), _p(n),
                  _p(mult), _p(user_log), _p(status), _stream())
        bits = int(status[0])
        if bits:
            raise RuntimeError(f"sessionize: the kernels skipped an index that was out of range (status {bits})")
        host = lambda v: v.cpu().numpy()
        user_dense = order_dense[host(user_log).astype(np.int64)] if U else order_dense[:0]
        return _result(host(seq), host(offsets), host(users_new), host(n), host(mult), host(train).astype(bool), host(kept), user_dense,
                       order_dense, lookups, host(poi_log), host(cat_log), lat, lon, poi, cat)
