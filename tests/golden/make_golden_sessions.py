"""G12: check-in SESSIONS and the trajectory dicts the reference makes of them (gen_pickles.py:735-833,
gen_poigraph_d1228_nyc_avg_maxtime) -- only possible where the reference is mounted, like the other generators.

The reference's function is run as it is, on seeded sessions.  Two shims make it importable and runnable today:
  * `train` (gen_pickles.py:5 imports two names from the reference's trainer, which needs packages that are not installed)
    is an empty stand-in in sys.modules -- the function under test uses neither name;
  * `gen_pickles.pd` is a proxy of pandas whose DataFrame turns a `set` given as index / columns into a list: current pandas
    refuses sets there ("index cannot be a set"), the pandas the reference was written for took them.  The frame is reindexed
    by node order afterwards (:817-818), so the order the set is listed in does not reach the output.

Stored in tests/golden/g12_sessions.npz, as flat arrays with offsets: the sessions (user, check-ins) and every field of every
dict the reference wrote.  Data only.

    python tests/golden/make_golden_sessions.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/graphormer"
SEED = 1228


def crafted():
    """(name, POIs of the whole session, target last) -- time slots and categories are drawn below unless given"""
    return [
        ("issue_example", [1, 4, 2, 1, 4, 4, 4, 4, 2], None),
        ("two_checkins", [7, 9], None),                                   # one node, no edge
        ("one_poi_repeated", [5] * 12 + [3], None),                       # one node, self-loop count L - 1
        ("no_repeats", list(range(10, 31)) + [4], None),
        ("ends_on_revisit", [3, 8, 5, 9, 8, 2, 3, 6], None),              # history ends on POI 3, visited first
        ("slots_0_and_47", [11, 12, 13, 11, 14, 12, 15], [0, 47, 0, 47, 0, 0, 47]),
        ("revisit_overwrites_slot", [21, 22, 21, 22, 21, 30], [5, 0, 47, 9, 0, 1]),
    ]


def sessions():
    rng = np.random.RandomState(SEED)
    out = []
    for name, pois, slots in crafted():
        pois = np.asarray(pois, dtype=np.int64)
        slots = rng.randint(0, 48, size=len(pois)) if slots is None else np.asarray(slots, dtype=np.int64)
        out.append((name, np.stack([pois, slots, rng.randint(1, 300, size=len(pois))], 1)))
    for P in (5, 50, 100000):
        for L in (2, 17, 64, 150, 300):
            pois = rng.randint(1, P + 1, size=L + 1)
            out.append((f"random_P{P}_L{L}", np.stack([pois, rng.randint(0, 48, size=L + 1), rng.randint(1, 300, size=L + 1)], 1)))
    users = rng.permutation(len(out)) * 3 + 1                             # distinct: the reference keys its output by user
    return [(n, int(u), c.astype(np.int64)) for (n, c), u in zip(out, users)]


def reference_function():
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
    sys.modules.setdefault("train", types.SimpleNamespace(RnnParameterData=None, generate_input_history=None))
    sys.path.insert(0, REF)
    import gen_pickles
    gen_pickles.pd = _Pandas()
    return gen_pickles.gen_poigraph_d1228_nyc_avg_maxtime


def main():
    fn = reference_function()
    sess = sessions()
    data = {}
    for i, (_, user, c) in enumerate(sess):
        # a check-in of the reference: [poi, time slot, lon, lat, ..., category] (:757-758, :763-764)
        rows = [[int(p), int(t), 0.0, 0.0, int(k)] for p, t, k in c]
        data[user] = {"sessions": {i: rows}, "train": [i], "test": []}
    ref = fn(data, "train")
    dicts = [ref[user][i] for i, (_, user, _) in enumerate(sess)]
    out = {"names": np.array([n for n, _, _ in sess]), "users": np.array([u for _, u, _ in sess], dtype=np.int64),
           "checkins": np.concatenate([c for _, _, c in sess]),
           "offsets": np.cumsum([0] + [len(c) for _, _, c in sess]).astype(np.int64),
           "node_offsets": np.cumsum([0] + [int(d["node_name"].numel()) for d in dicts]).astype(np.int64),
           "edge_offsets": np.cumsum([0] + [int(d["edge_type"].numel()) for d in dicts]).astype(np.int64)}
    for k in ("node_name", "edge_type", "time", "time_normal", "cat", "target", "user"):
        out["ref_" + k] = np.concatenate([d[k].numpy().reshape(-1) for d in dicts])
    out["ref_num_node"] = np.array([d["num_node"] for d in dicts], dtype=np.int64)
    assert out["ref_time_normal"].dtype == np.float32 and out["ref_edge_type"].dtype == np.int64
    path = os.path.join(HERE, "g12_sessions.npz")
    np.savez_compressed(path, **out)
    print(f"wrote g12_sessions.npz: {os.path.getsize(path) / 1024:.0f} KB, {len(sess)} sessions, "
          f"n up to {int(out['ref_num_node'].max())}")


if __name__ == "__main__":
    main()
