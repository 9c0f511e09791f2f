"""G14: a raw check-in log and the sessions the reference's offline preprocessing makes of it (graphormer/foursquare_process.py:
load_trajectory_from_tweets :115-180, filter_users_by_length :183-259, build_users_locations_dict :262-294, load_venues :297-310,
venues_lookup :313-319, prepare_neural_data :377-482).  Only possible where the reference is mounted, like the other generators.

The reference's six methods are run as they are, under TZ=UTC and with a log whose offset column is 0 (its wall clock goes
through mktime / localtime: with both it is calendar.timegm of the log's time string), on a seeded log of about 2 000 lines in
the TSMC2014 tab format written to a temporary file that a DataFoursquare's TWITTER_PATH points at.  The shims are
make_golden_universe.py's (a pandas proxy, an identity tqdm); so is write_npz.

The log is run twice: sorted by time, and shuffled inside blocks of BLOCK lines (the reference does not sort: a user's records are cut in log order, and a
negative gap is legal).  It holds, asserted below: a user below trace_min; a POI below global_visit; a user whose kept sessions
fall short of sessions_min; two surviving users with equal counts; a session that fills and forces a start under min_gap; gaps
of exactly 86 400 / 86 399 / 600 / 599 s; a POI logged under two categories; users with more than 64 and more than 128
remaining records.  Latitude and longitude differ from line to line of a POI in the sixth decimal, so that WHICH check-in gives
a POI its coordinates shows.

Stored in tests/golden/g14_checkins.npz, data only: the log's columns (user, poi, cat as strings, t, lat, lon) and the
permutation of the shuffled copy; per copy (prefixes sorted_ / shuffled_) the dense sessions the reference built (data_neural:
seq rows (poi, slot, category), offsets, users, train), the raw ids in uid_list / vid_list / catid_list order and the first-seen
lat / lon of vid_list.

    python tests/golden/make_golden_checkins.py
"""
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_universe import reference_module, write_npz  # noqa: E402

SEED = 1414
T0 = 1333238400                                    # 2012-04-01 00:00:00 UTC
N_POPULAR, N_RARE, N_CAT = 40, 60, 9
BLOCK = 12                                         # lines of the log that the shuffled copy permutes among themselves
PARAMS = dict(trace_min=10, global_visit=10, hour_gap=24, min_gap=10, session_min=5, session_max=10, sessions_min=2, train_split=0.8)


def make_log():
    """-> the time-sorted log as columns: user, poi, cat (strings), t (int64 seconds), lat, lon (float64, 6 decimals)"""
    rng = np.random.RandomState(SEED)
    pids = ["4b%010x" % v for v in rng.choice(16 ** 8, size=N_POPULAR + N_RARE, replace=False)]
    cats = ["4bf58dd8d48988d1%02x931735" % v for v in rng.choice(256, size=N_CAT, replace=False)]
    cat_of = rng.randint(0, N_CAT, size=len(pids))
    lat0, lon0 = 35.68 + 0.03 * rng.randn(len(pids)), 139.76 + 0.04 * rng.randn(len(pids))
    rows = []                                                          # (user, poi index, t, category index)

    def visit(user, t, p=None, popular=False):
        if p is None:
            p = (rng.randint(0, 10) if popular else rng.randint(0, N_POPULAR) if rng.rand() < 0.88
                 else N_POPULAR + rng.randint(0, N_RARE))              # (the crafted users visit the ten most visited POIs)
        c = cat_of[p]
        if p == 3 and rng.rand() < 0.5:
            c = (c + 1) % N_CAT                                        # POI 3 is logged under two categories
        rows.append((user, p, int(t), c))

    # seeded users: steps of 15 - 90 min (append), 2 - 8 min (dropped) and 25 - 60 h (a new session)
    for k, count in enumerate([330, 280, 180, 140, 140, 120, 100, 90, 90, 70, 60, 60, 48, 40, 32, 24, 16, 12]):
        t = T0 + rng.randint(0, 86400 * 3)
        for _ in range(count):
            visit("u%03d" % (100 + k), t)
            kind = rng.rand()
            t += rng.randint(900, 5400) if kind < 0.72 else rng.randint(120, 480) if kind < 0.82 else rng.randint(25 * 3600, 60 * 3600)
    # below trace_min
    for k in range(4):
        visit("tiny", T0 + 1000 * k, popular=True)
    # one kept session only: short of sessions_min
    for k in range(12):
        visit("once", T0 + 5000 + 1200 * k, popular=True)
    # a session that fills (session_max + 1 = 11 records), a record 60 s later that starts the next, which is kept
    t = T0 + 7000
    for k in range(11):
        visit("full", t, popular=True)
        t += 900
    t += 60 - 900
    for k in range(6):
        visit("full", t, popular=True)
        t += 900
    # the thresholds, to the second: 5 records; + 86 399 s appends; + 86 400 s starts; + 600 s appends; + 599 s is dropped; 4 more
    t = T0 + 9000
    for step in [900, 900, 900, 900, 86399, 86400, 600, 599, 900, 900, 900, 900, 0]:
        visit("edge", t, popular=True)
        t += step
    rows.sort(key=lambda r: r[2])                                      # (stable)
    lat = np.array([round(lat0[p] + 1e-6 * (i % 7), 6) for i, (_, p, _, _) in enumerate(rows)])
    lon = np.array([round(lon0[p] + 1e-6 * (i % 5), 6) for i, (_, p, _, _) in enumerate(rows)])
    return dict(user=np.array([r[0] for r in rows]), poi=np.array([pids[r[1]] for r in rows]), cat=np.array([cats[r[3]] for r in rows]),
                t=np.array([r[2] for r in rows], dtype=np.int64), lat=lat, lon=lon)


def write_log(path, log, order):
    with open(path, "w", encoding="utf-8") as f:
        for i in order:
            stamp = time.strftime("%a %b %d %H:%M:%S +0000 %Y", time.gmtime(int(log["t"][i])))
            f.write("\t".join([log["user"][i], log["poi"][i], log["cat"][i], "Some Venue", "%.6f" % log["lat"][i], "%.6f" % log["lon"][i],
                               "0", stamp]) + "\n")


def run_reference(fp, path):
    ref = fp.DataFoursquare(**PARAMS)
    ref.TWITTER_PATH = path
    ref.load_trajectory_from_tweets()
    ref.filter_users_by_length()
    ref.build_users_locations_dict()
    ref.load_venues()
    ref.venues_lookup()
    ref.prepare_neural_data()
    return ref


def extract(ref):
    seq, offsets, users, train = [], [0], [], []
    for u in ref.uid_list:
        uid = ref.uid_list[u][0]
        d = ref.data_neural[uid]
        assert list(d["sessions"]) == list(range(len(d["sessions"])))
        for sid, rows in d["sessions"].items():
            seq += [[r[0], r[1], r[-1]] for r in rows]
            offsets.append(len(seq))
            users.append(uid)
            train.append(sid in d["train"])
    P, n_cat = len(ref.vid_list) - 1, len(ref.catid_list) - 1
    vids = [ref.vid_list_lookup[k] for k in range(1, P + 1)]
    return dict(seq=np.array(seq, dtype=np.int64), offsets=np.array(offsets, dtype=np.int64), users=np.array(users, dtype=np.int64),
                train=np.array(train), uid_order=np.array(list(ref.uid_list)), vid_order=np.array(vids),
                cat_order=np.array([ref.catid_list_lookup[k] for k in range(1, n_cat + 1)]),
                coords=np.array([[float(ref.vid_list[p][2]), float(ref.vid_list[p][3])] for p in vids], dtype=np.float64))


def check_sorted(ref, log):
    """What the log is for, read off the reference's own state of the time-sorted run."""
    p = PARAMS
    counts = {u: len(v) for u, v in ref.data.items()}
    assert counts["tiny"] < p["trace_min"] and "tiny" not in ref.uid_list
    assert min(ref.venues.values()) < p["global_visit"] <= max(ref.venues.values())
    assert counts["once"] >= p["trace_min"] and "once" not in ref.data_filter and "once" not in ref.uid_list
    survivors = list(ref.uid_list)
    by_count = [counts[u] for u in survivors]
    assert by_count == sorted(by_count, reverse=True) and len(set(by_count)) < len(by_count)          # ties, in first-seen order
    tied = [u for u in survivors if by_count.count(counts[u]) > 1]
    first_seen = {u: i for i, u in enumerate(ref.data)}
    assert all(first_seen[a] < first_seen[b] for a, b in zip(tied, tied[1:]) if counts[a] == counts[b])
    stamp = lambda r: int(time.mktime(time.strptime(r[1], "%Y-%m-%d %H:%M:%S")))
    raw = ref.data_filter["full"]["raw_sessions"]
    assert len(raw[0]) == p["session_max"] + 1 and stamp(raw[1][0]) - stamp(raw[0][-1]) == 60 < 60 * p["min_gap"]
    assert len(raw[1]) >= p["session_min"]
    edge = ref.data_filter["edge"]["raw_sessions"]
    assert [len(s) for s in edge.values()] == [6, 6]
    te = [stamp(r) for s in edge.values() for r in s]
    assert te[5] - te[4] == 86399 and te[6] - te[5] == 86400 and te[7] - te[6] == 600 and te[8] - te[7] == 599 + 900
    kept_poi = {v for v, c in ref.venues.items() if c >= p["global_visit"]}
    remaining = sorted(sum(r[0] in kept_poi for r in ref.data[u]) for u in survivors)
    assert remaining[-1] > 128 and any(64 < r <= 128 for r in remaining) and any(r < 64 for r in remaining), remaining
    cats_of = {}
    for u in survivors:
        for s in ref.data_filter[u]["sessions"].values():
            for r in s:
                cats_of.setdefault(r[0], set()).add(r[-1])
    assert max(len(c) for c in cats_of.values()) == 2
    lens = [len(s) for u in survivors for s in ref.data_filter[u]["sessions"].values()]
    assert max(lens) == p["session_max"] + 1 and min(lens) == p["session_min"]
    assert len({len(ref.data_filter[u]["sessions"]) for u in survivors}) >= 4


def main():
    os.environ["TZ"] = "UTC"
    time.tzset()
    fp = reference_module()
    log = make_log()
    N = len(log["t"])
    rng = np.random.RandomState(SEED + 1)                              # shuffled inside blocks: sessions still form
    perm = np.concatenate([a + rng.permutation(min(BLOCK, N - a)) for a in range(0, N, BLOCK)])
    out = dict(log, perm=perm.astype(np.int64))
    with tempfile.TemporaryDirectory() as tmp:
        for name, order in (("sorted", np.arange(N)), ("shuffled", perm)):
            path = os.path.join(tmp, name + ".txt")
            write_log(path, log, order)
            ref = run_reference(fp, path)
            if name == "sorted":
                check_sorted(ref, log)
            got = extract(ref)
            assert len(got["users"]) >= 20 and not got["train"].all() and got["train"].any(), (name, len(got["users"]))
            out.update({f"{name}_{k}": v for k, v in got.items()})
    assert not np.array_equal(out["sorted_seq"], out["shuffled_seq"]) and (np.diff(log["t"][perm]) < 0).any()
    for k in ("user", "poi", "cat", "sorted_uid_order", "sorted_vid_order", "sorted_cat_order"):
        assert out[k].dtype.kind == "U", k
    path = os.path.join(HERE, "g14_checkins.npz")
    write_npz(path, out)
    print(f"wrote g14_checkins.npz: {os.path.getsize(path) / 1024:.0f} KB, {N} lines; "
          + "; ".join(f"{name}: {len(out[name + '_uid_order'])} users, {len(out[name + '_users'])} sessions "
                      f"({int(out[name + '_train'].sum())} train), {len(out[name + '_seq'])} check-ins, {len(out[name + '_vid_order'])} POIs, "
                      f"{len(out[name + '_cat_order'])} categories" for name in ("sorted", "shuffled")))


if __name__ == "__main__":
    main()
