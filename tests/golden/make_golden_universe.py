"""G13: check-in sessions and the four files the reference's offline preprocessing makes of them -- Graph_poi.csv,
Graph_cat.csv, Graph_adj.csv and Graph_dist.csv (graphormer/foursquare_process.py: build_users_locations_dict :262-294,
venues_lookup :313-319, prepare_neural_data :377-491, prepare_global_data :565-754).  Only possible where the reference is
mounted, like the other generators.

The reference's four methods are run as they are on seeded raw sessions (what its raw-log filters, :115-260, would leave in
data_filter): 12 users with 2 .. 8 sessions each (a user with two sessions has a single train session), about 150 POIs with
string ids, 12 categories.  Two shims make them run today:
  * `foursquare_process.pd` is a proxy of pandas whose DataFrame turns a `set` given as index / columns into a list: current
    pandas refuses sets there, the pandas the reference was written for took them (make_golden_sessions.py has the same shim);
  * `foursquare_process.tqdm` is the identity, which keeps the progress bars out of the output (whether the reference needs
    that to run was not checked).
The process works in a temporary directory that has ../dataset/foursquaregraph/raw/, where the reference writes.

The coordinates are drawn so that no POI pair lies within 1e-6 km of the 3 km radius or of another POI (asserted below, with
the reference's own LLs2Dist): Graph_dist cannot depend on which f64 formula of the distance decides it.

Stored in tests/golden/g13_universe.npz, data only: the dense integer sessions the reference built (data_neural), their users
and train flags; the coordinates; the raw id sequences (for data.first_seen_ids); the four files' arrays as pd.read_csv returns
them.  The archive is written with fixed timestamps, so a second run reproduces the file bit for bit.

    python tests/golden/make_golden_universe.py
"""
import io
import os
import sys
import tempfile
import types
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/graphormer"
SEED = 1313
N_USERS, POOL, N_CAT = 12, 165, 12
MARGIN_KM = 1e-6


def raw_sessions():
    """-> (data_filter {user: {"sessions": {sid: [[pid, time string, lat, lon, category id], ...]}}}, user order,
    pid_loc_lat {pid: [lon, lat]})"""
    rng = np.random.RandomState(SEED)
    pids = np.array(["4b%010x" % v for v in rng.choice(16 ** 8, size=POOL, replace=False)])
    cats = np.array(["4bf58dd8d48988d1%02x931735" % v for v in rng.choice(256, size=N_CAT, replace=False)])
    cat_of = rng.randint(0, N_CAT, size=POOL)
    cat_of[:N_CAT] = rng.permutation(N_CAT)                            # every category occurs among the popular POIs
    lat = 35.68 + 0.03 * rng.randn(POOL)
    lon = 139.76 + 0.04 * rng.randn(POOL)
    weight = 1.0 / np.arange(1, POOL + 1) ** 0.35                      # a few popular POIs, a long tail
    weight /= weight.sum()
    n_sessions = [2, 2, 3, 5, 5, 6, 8, 4, 2, 7, 5, 6]
    assert len(n_sessions) == N_USERS
    data_filter, users = {}, []
    for u in range(N_USERS):
        user = "u%04d" % rng.randint(0, 10000)
        assert user not in data_filter
        users.append(user)
        sessions = {}
        for sid in range(n_sessions[u]):
            length = int(rng.randint(2, 11))
            pois = rng.choice(POOL, size=length, p=weight)
            if rng.rand() < 0.4:
                pois[rng.randint(1, length)] = pois[0]                 # a revisit, and a self transition where they touch
            rows = []
            for p in pois:
                stamp = "2012-%02d-%02d %02d:%02d:%02d" % (rng.randint(4, 7), rng.randint(1, 29), rng.randint(0, 24), rng.randint(0, 60),
                                                           rng.randint(0, 60))
                rows.append([str(pids[p]), stamp, float(lat[p]), float(lon[p]), str(cats[cat_of[p]])])
            sessions[sid] = rows
        data_filter[user] = {"sessions_count": len(sessions), "sessions": sessions}
    return data_filter, users, {str(pids[p]): [float(lon[p]), float(lat[p])] for p in range(POOL)}


def reference_module():
    import pandas

    class _Pandas:
        def __getattr__(self, k):
            return getattr(pandas, k)

        @staticmethod
        def DataFrame(data=None, index=None, columns=None, **kw):
            index = list(index) if isinstance(index, (set, frozenset)) else index
            columns = list(columns) if isinstance(columns, (set, frozenset)) else columns
            return pandas.DataFrame(data, index=index, columns=columns, **kw)

    sys.dont_write_bytecode = True
    try:
        import tqdm  # noqa: F401
    except ImportError:
        sys.modules["tqdm"] = types.SimpleNamespace(tqdm=lambda it, *a, **k: it)
    sys.path.insert(0, REF)
    import foursquare_process as fp
    fp.pd = _Pandas()
    fp.tqdm = lambda it, *a, **k: it
    return fp


def write_npz(path, arrays):
    """np.savez_compressed with fixed timestamps: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    import pandas as pd
    fp = reference_module()
    data_filter, users, pid_loc_lat = raw_sessions()
    ref = fp.DataFoursquare()
    ref.data_filter, ref.user_filter3, ref.pid_loc_lat = data_filter, users, pid_loc_lat
    here = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        raw = os.path.join(tmp, "dataset", "foursquaregraph", "raw")
        os.makedirs(raw)
        os.makedirs(os.path.join(tmp, "work"))
        os.chdir(os.path.join(tmp, "work"))
        try:
            ref.build_users_locations_dict()
            ref.venues_lookup()
            ref.prepare_neural_data()
            ref.prepare_global_data()
        finally:
            os.chdir(here)
        frames = {k: pd.read_csv(os.path.join(raw, f"Graph_{k}.csv")) for k in ("poi", "cat", "adj", "dist")}
    P, n_cat = len(ref.vid_list) - 1, len(ref.catid_list) - 1
    for k, n in (("cat", n_cat), ("adj", P), ("dist", P)):                # headers 1 .. K, in that order: row i is id i + 1
        assert [int(c) for c in frames[k].columns] == list(range(1, n + 1)) and frames[k].shape == (n, n), k
    assert list(frames["poi"].columns) == ["POI ID", "checkin_cnt", "lat", "lon", "cat", "cat_freq"] and len(frames["poi"]) == P
    out = {"ref_" + k: f.to_numpy() for k, f in frames.items()}
    assert np.array_equal(out["ref_poi"][:, 0], np.arange(1, P + 1))

    # the dense sessions as the reference built them, users in uid_list order, and what it trains on
    seq, offsets, sess_user, train, raw_poi, raw_cat = [], [0], [], [], [], []
    for user in users:
        uid = ref.uid_list[user][0]
        d = ref.data_neural[uid]
        for sid, rows in d["sessions"].items():
            seq += [[r[0], r[1], r[-1]] for r in rows]
            offsets.append(len(seq))
            sess_user.append(uid)
            train.append(sid <= d["train"][-1])
            raw_poi += [r[0] for r in data_filter[user]["sessions"][sid]]
            raw_cat += [r[-1] for r in data_filter[user]["sessions"][sid]]
    train = np.array(train)
    per_user = np.bincount(np.array(sess_user)[train], minlength=len(users))
    assert per_user.min() == 1 and (per_user == 1).sum() >= 2 and not train.all()
    out.update(seq=np.array(seq, dtype=np.int64), offsets=np.array(offsets, dtype=np.int64), users=np.array(sess_user, dtype=np.int64),
               train=train, coords=np.ascontiguousarray(out["ref_poi"][:, 2:4]), raw_poi=np.array(raw_poi), raw_cat=np.array(raw_cat))
    assert out["raw_poi"].dtype.kind == "U" and out["seq"][:, 0].max() == P and out["seq"][:, 2].max() == n_cat

    # the margin: the reference's own distance of every pair stays away from the radius and from zero
    c = out["coords"]
    d = np.array([[fp.LLs2Dist(c[i, 0], c[i, 1], c[j, 0], c[j, 1]) for j in range(P)] for i in range(P)])
    off = ~np.eye(P, dtype=bool)
    assert np.abs(d - 3.0).min() > MARGIN_KM and d[off].min() > MARGIN_KM, (np.abs(d - 3.0).min(), d[off].min())
    assert np.array_equal(out["ref_dist"], ((d <= 3.0) & (d > 0)).astype(np.float64))

    path = os.path.join(HERE, "g13_universe.npz")
    write_npz(path, out)
    n_train = int(np.diff(out["offsets"])[train].sum() - train.sum())
    print(f"wrote g13_universe.npz: {os.path.getsize(path) / 1024:.0f} KB, {len(users)} users, {len(train)} sessions ({int(train.sum())} "
          f"train), {len(seq)} check-ins, {P} POIs, {n_cat} categories, {n_train} train transitions, "
          f"{int(out['ref_dist'].sum())} within-radius pairs")


if __name__ == "__main__":
    main()
