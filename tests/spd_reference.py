"""Reference side of the shortest-path preprocessing matrix (tests/test_gpu_spd_matrix.py, tests/test_host_spd_reference.py): the
case list as plain data, the graph builders, the expected outputs of every entry point of csrc/spd.hip derived from the committed
oracle (oracle/algos_oracle.py, pinned bit for bit to the reference's Cython build by tests/golden/g1_algos.npz) exactly as
include/mobgt_hip.h states them, a second restatement of the path walk that shares nothing with the kernel's algorithm, the wrong
references (MUTANTS) the verdicts must reject, and the verdicts.  All of it is integer data: every comparison is np.array_equal
over the whole array, padding included.  NumPy and the oracle only; never the code under test.

Expected outputs of mobgt_spd_batched for a graph of n nodes inside an N-wide slot (M, path = ao.floyd_warshall(counts != 0)):
    spd      M on real pairs, -1 on padding                     path     path on real pairs, -1 on padding
    rel_pos  M + 1 on real pairs, 0 on padding                  degrees  row sum + 1 ("in") / column sum + 1 ("out"), 0 on padding
    edge_input[i, j, d] = feature of the d-th hop of the walk i -> j for d < min(hops, D), 0 behind it, on i == j, on unreachable
             pairs and on padding; the feature of a hop (a, b) is count + 3 saturated at 255 on an edge and 1 on a non-edge (a
             shortest path through node 0 loses node 0: the reference's quirk, kept).
"First D hops" is oracle_gen_edge_input called at max_dist = D through ao._lib(): the C loop writes the first max_dist hops of a
pair before it reports 1 (only the Python wrapper raises), so return codes 0 and 1 are both accepted.
The padding rows and columns of `counts` hold PAD_COUNT: the contract says they are ignored."""
import ctypes
import os
import zlib

import numpy as np

from mobgt_amd import _lib, synth
from oracle import algos_oracle as ao

C = _lib.CONSTANTS
LDS_MAX_N, SPLIT_MAX_N, SPLIT_PARTS, MAX_D = (C["MOBGT_SPD_" + n] for n in ("LDS_MAX_N", "SPLIT_MAX_N", "SPLIT_PARTS", "MAX_D"))
UNREACH = 510
SAT_COUNTS = (1, 2, 249, 250, 251, 252, 253, 254, 255, 1000, 2 ** 31 - 1)
PAD_COUNT = 7
POISON_U8 = 0xA5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g1_algos.npz")
FIELDS = ("spd", "path", "rel_pos", "edge_input", "in_degree", "out_degree")


# ------------------------------------------------------------------------------------------------ graphs
def _rng(*key):
    return np.random.RandomState(zlib.crc32("/".join(str(k) for k in key).encode()))


_GOLD = {}


def golden(name):
    if not _GOLD:
        z = np.load(GOLDEN)
        for nm in z["names"]:
            _GOLD[str(nm)] = {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(f"{nm}/")}
    return _GOLD[name]


def golden_names():
    golden("chain5")
    return list(_GOLD)


def _edges(n, pairs):
    c = np.zeros((n, n), np.int64)
    for a, b in pairs:
        c[a, b] = 1
    return c


def _mid0_perm(rng, n):
    p = rng.permutation(np.arange(1, n))
    return np.concatenate([p[:n // 2], [0], p[n // 2:]])


FAMILIES = {
    "empty": lambda rng, n: np.zeros((0, 0), np.int64),
    "single": lambda rng, n: np.zeros((1, 1), np.int64),
    "loop": lambda rng, n: np.ones((1, 1), np.int64),
    "noedge": lambda rng, n: np.zeros((n, n), np.int64),
    "chain": lambda rng, n: _edges(n, [(i, i + 1) for i in range(n - 1)]),                  # path[i][j] = j - 1: the deepest stack
    "rchain": lambda rng, n: _edges(n, [(i + 1, i) for i in range(n - 1)]),                 # path[i][j] = i - 1: the shallowest
    "pchain": lambda rng, n: (lambda p: _edges(n, [(p[i], p[i + 1]) for i in range(n - 1)]))(rng.permutation(n)),
    "cycle": lambda rng, n: _edges(n, [(i, (i + 1) % n) for i in range(n)]),
    "star0": lambda rng, n: _edges(n, [(0, i) for i in range(1, n)] + [(i, 0) for i in range(1, n)]),
    "mid0": lambda rng, n: (lambda p: _edges(n, [(p[i], p[i + 1]) for i in range(n - 1)]))(_mid0_perm(rng, n)),
    "complete": lambda rng, n: 1 - np.eye(n, dtype=np.int64),
    "twocomp": lambda rng, n: _edges(n, [(i, i + 1) for i in range(n - 1) if i + 1 != n // 2] + [(n - 1, n // 2)]),  # a chain, a cycle
    "loops": lambda rng, n: np.maximum(synth.random_digraph(rng, n, min(0.5, 2.5 / n)), np.eye(n, dtype=np.int64)),
    "rand": lambda rng, n: synth.random_digraph(rng, n, min(0.5, 4.0 / max(n, 1))),
    "traj": lambda rng, n: synth.make_trajectory(rng, 2000, n, 4)["edge_type"],
}


def g(fam, n=0, sat=False, seed=0):
    """A graph spec: the family, its node count, whether its counts are redrawn from SAT_COUNTS, a seed."""
    return (fam, int(n), bool(sat), int(seed))


def gid(spec):
    fam, n, sat, seed = spec
    return fam + (str(n) if n else "") + ("s" if sat else "") + (f"#{seed}" if seed else "")


_GRAPH, _FW = {}, {}


def graph(spec):
    """The int64 count matrix [n, n] of a spec (built once, never modified)."""
    if spec not in _GRAPH:
        fam, n, sat, seed = spec
        rng = _rng("spd", *spec)
        c = golden(fam[7:])["counts"].astype(np.int64) if fam.startswith("golden:") else np.asarray(FAMILIES[fam](rng, n), np.int64)
        if sat:
            c = c.copy()
            nz = np.flatnonzero(c)
            c.flat[nz] = rng.choice(np.asarray(SAT_COUNTS, np.int64), nz.size)
            if nz.size >= len(SAT_COUNTS):                                      # (every listed count at least once)
                c.flat[nz[rng.permutation(nz.size)[:len(SAT_COUNTS)]]] = SAT_COUNTS
        assert c.ndim == 2 and c.shape[0] == c.shape[1] and (c >= 0).all() and c.max(initial=0) < 2 ** 31
        c.setflags(write=False)
        _GRAPH[spec] = c
    return _GRAPH[spec]


def fw(spec):
    """(M, path) int64 of ao.floyd_warshall(counts != 0), cached."""
    if spec not in _FW:
        c = graph(spec)
        _FW[spec] = ao.floyd_warshall(c != 0) if c.shape[0] else (np.zeros((0, 0), np.int64), np.zeros((0, 0), np.int64))
    return _FW[spec]


# ------------------------------------------------------------------------------------------------ the oracle, tolerant of rc 1
def first_hops(path, feat, D):
    """float32 [n, n, D, F]: oracle_gen_edge_input at max_dist = D.  0: no path is longer than D; 1: some are, and their first D
    hops stand in the output (oracle/algos_ref.c:93-98).  Anything else is an error."""
    path = np.ascontiguousarray(np.asarray(path, np.int64))
    feat = np.ascontiguousarray(np.asarray(feat, np.int64))
    n, F = path.shape[0], feat.shape[-1]
    out = np.empty((n, n, int(D), F), np.float32)
    if n == 0 or D == 0:
        return out
    p = lambda a, t: a.ctypes.data_as(ctypes.POINTER(t))                                     # noqa: E731
    rc = ao._lib().oracle_gen_edge_input(int(D), p(path, ctypes.c_int64), p(feat, ctypes.c_int64), n, F, p(out, ctypes.c_float))
    assert rc in (0, 1), rc
    return out


def feature(c, mut=None):
    """The uint8 hop feature of every pair of a count matrix."""
    c = np.asarray(c, np.int64)
    if mut == "sat_252":
        f = np.minimum(c + 3, 252)
    elif mut == "sat_wrap":
        f = (c + 3) & 255
    else:
        f = np.where(c > 252, 255, c + 3)
    return np.where(c != 0, f, 1)


# ------------------------------------------------------------------------------------------------ the independent restatement
def prefix_hops(P, D, M=None, fix0=False, unreach=UNREACH):
    """{(i, j): the first D hops (a, b) of the walk i -> j} for every i != j whose path entry is not the sentinel, by a memoised
    prefix: prefix(i, j) = (prefix(i, k) + prefix(k, j))[:D] with k = path[i][j], and k == 0 a leaf.  fix0 (a mutant): a pair is a
    leaf only where M <= 1, so an intermediate node 0 is expanded."""
    n = P.shape[0]
    Pl = np.asarray(P).tolist()
    memo = {}

    def prefix(i, j):
        r = memo.get((i, j))
        if r is None:
            k = Pl[i][j]
            leaf = (i == j or M[i][j] <= 1) if fix0 else k == 0
            r = ((i, j),) if leaf else (prefix(i, k) + prefix(k, j))[:D]
            memo[(i, j)] = r
        return r
    return {(i, j): prefix(i, j) for i in range(n) for j in range(n) if i != j and Pl[i][j] != unreach}


def lifo_hops(P, D, drop_newest=False, unreach=UNREACH):
    """The same set by the kernel's own algorithm (a ring of D pending targets whose oldest entry is overwritten, the same guard):
    the header's claim that dropping the oldest never changes the first D hops is checked with it, and the mutants with a wrong
    path matrix or a wrong ring are built on it."""
    n = P.shape[0]
    Pl = np.asarray(P).tolist()
    out = {}
    for i in range(n):
        for j in range(n):
            if i == j or Pl[i][j] == unreach:
                continue
            hops, ring, size, top, a, guard = [], [0] * D, 1, 0, i, 4 * n + 2 * D + 8
            ring[0] = j
            while len(hops) < D and size > 0 and guard > 0:
                guard -= 1
                t = ring[top]
                k = Pl[a][t]
                if k == 0:
                    hops.append((a, t))
                    a = t
                    top = D - 1 if top == 0 else top - 1
                    size -= 1
                elif k >= n:                             # (only a mutant's path matrix: the sentinel as a sub-pair)
                    break
                elif drop_newest and size == D:          # (the mutant ring: full, the push is lost)
                    pass
                else:
                    top = 0 if top == D - 1 else top + 1
                    ring[top] = k
                    size = min(size + 1, D)
            out[(i, j)] = tuple(hops)
    return out


def hops_array(hops, feat, n, D, behind=0):
    """uint8 [n, n, D] of a hop set: feat[a, b] per hop, `behind` behind the last hop of a walked pair, 0 on every other pair."""
    out = np.zeros((n, n, D), np.int64)
    for (i, j), hs in hops.items():
        out[i, j, len(hs):] = behind
        for d, (a, b) in enumerate(hs):
            out[i, j, d] = feat[a, b]
    return out.astype(np.uint8)


def np_fw(adj, mut=None):
    """algos.pyx:9-54 in NumPy, one vectorised step per k (row k and column k do not change inside step k), with the Floyd-Warshall
    mutants: `>=` for `>`; row k read as it stood before step k - 1; sentinel 511; path left alone on unreachable pairs."""
    n = adj.shape[0]
    S = 511 if mut == "sentinel_511" else UNREACH
    M = np.where(adj != 0, 1, S).astype(np.int64)
    M[np.arange(n), np.arange(n)] = 0
    P = np.zeros((n, n), np.int64)
    before_prev = M.copy()
    for k in range(n):
        start = M.copy()
        rowk = before_prev[k] if (mut == "jacobi_step" and k > 0) else start[k]
        c = start[:, k, None] + rowk[None, :]
        upd = (M >= c) if mut == "ge_first_k" else (M > c)
        M = np.where(upd, c, M)
        P[upd] = k
        before_prev = start
    far = M >= S
    M[far] = S
    if mut != "path_unset_unreach":
        P[far] = S
    return M, P


# ------------------------------------------------------------------------------------------------ mobgt_spd_batched, expected
FW_MUTANTS = ("ge_first_k", "jacobi_step", "sentinel_511", "path_unset_unreach")
HOP_MUTANTS = ("node0_fixed", "hops_reversed", "ring_drops_newest", "sat_252", "sat_wrap", "edge_input_not_zeroed")
PAD_MUTANTS = ("degrees_swapped", "rel_pos_pad_as_real")
COLLATE_MUTANTS = ("cut_gt", "cut_above_510", "poi_pos_x0", "col_n_not_key", "col_n1_key")
MUTANTS = FW_MUTANTS + HOP_MUTANTS + PAD_MUTANTS + COLLATE_MUTANTS

_PARTS = {}


def graph_outputs(spec, D, mut=None):
    """The unpadded outputs of one graph: M, path int64 [n, n]; hops uint8 [n, n, D]; ind, outd int64 [n]."""
    key = (spec, D)
    if mut is None and key in _PARTS:
        return _PARTS[key]
    c = graph(spec)
    n = c.shape[0]
    adj = c != 0
    M, P = np_fw(adj, mut) if mut in FW_MUTANTS else fw(spec)
    feat = feature(c, mut)
    sentinel = 511 if mut == "sentinel_511" else UNREACH
    if mut in FW_MUTANTS or mut == "ring_drops_newest":
        hops = hops_array(lifo_hops(P, D, mut == "ring_drops_newest", sentinel), feat, n, D)
    elif mut == "node0_fixed":
        hops = hops_array(prefix_hops(P, D, M=M.tolist(), fix0=True), feat, n, D)
    elif mut == "hops_reversed":
        hops = hops_array({k: h[::-1] for k, h in prefix_hops(P, D).items()}, feat, n, D)
    elif mut == "edge_input_not_zeroed":
        hops = hops_array(prefix_hops(P, D), feat, n, D, behind=POISON_U8)
    else:
        ei = first_hops(P, feat[:, :, None], D)[..., 0]
        hops = np.where(ei == -1, 0, ei).astype(np.uint8)
    r = dict(M=M, path=P, hops=hops, ind=adj.sum(1) + 1, outd=adj.sum(0) + 1)
    if mut is None:
        _PARTS[key] = r
    return r


def batch_inputs(case):
    """counts int32 [G, N, N] (PAD_COUNT outside a graph's block) and n_nodes int32 [G] of a batched case."""
    N = case["N"]
    counts = np.full((len(case["graphs"]), N, N), PAD_COUNT, np.int32)
    n_nodes = np.zeros(len(case["graphs"]), np.int32)
    for k, spec in enumerate(case["graphs"]):
        c = graph(spec)
        n = c.shape[0]
        assert n <= N
        counts[k, :n, :n] = c
        n_nodes[k] = n
    return counts, n_nodes


_EXPECTED = {}


def expected_batched(case, mut=None):
    """{field: the whole padded array} of a batched case, cached for mut = None (the work mode does not enter)."""
    key = (tuple(case["graphs"]), case["N"], case["D"])
    if mut is None and key in _EXPECTED:
        return _EXPECTED[key]
    G, N, D = len(case["graphs"]), case["N"], case["D"]
    i16 = np.int16
    e = dict(spd=np.full((G, N, N), -1, i16), path=np.full((G, N, N), -1, i16), rel_pos=np.zeros((G, N, N), i16),
             edge_input=np.zeros((G, N, N, D), np.uint8), in_degree=np.zeros((G, N), i16), out_degree=np.zeros((G, N), i16))
    if mut == "rel_pos_pad_as_real":                    # padded nodes as isolated real ones: 510 + 1 off the diagonal, 0 + 1 on it
        e["rel_pos"][:] = UNREACH + 1
        e["rel_pos"][:, np.arange(N), np.arange(N)] = 1
    for k, spec in enumerate(case["graphs"]):
        r = graph_outputs(spec, D, mut)
        n = r["M"].shape[0]
        e["spd"][k, :n, :n] = r["M"]
        e["path"][k, :n, :n] = r["path"]
        e["rel_pos"][k, :n, :n] = r["M"] + 1
        e["edge_input"][k, :n, :n] = r["hops"]
        a, b = ("outd", "ind") if mut == "degrees_swapped" else ("ind", "outd")
        e["in_degree"][k, :n] = r[a]
        e["out_degree"][k, :n] = r[b]
    if mut is None:
        for v in e.values():
            v.setflags(write=False)
        _EXPECTED[key] = e
    return e


def judge(want, got, names=None):
    """(ok, message): np.array_equal of every field over the whole array; the message names the field, the first differing index
    (the graph first) and both values."""
    for f, w in want.items():
        x = np.asarray(got[f])
        if x.shape != w.shape:
            return False, f"{f}: shape {x.shape}, expected {w.shape}"
        if not np.array_equal(x, w):
            at = tuple(int(v) for v in np.argwhere(x != w)[0])
            who = f" (graph {names[at[0]]})" if names is not None else ""
            return False, f"{f}{list(at)}{who}: got {x[at]}, expected {w[at]}; {int((x != w).sum())} elements differ"
    return True, ""


def branch(N, with_work):
    """Which Floyd-Warshall kernel mobgt_spd_batched takes (the dispatch of csrc/spd.hip, from the header's thresholds)."""
    if N <= LDS_MAX_N:
        return "lds"
    return "split" if N <= SPLIT_MAX_N and with_work else "global"


# ------------------------------------------------------------------------------------------------ the case list
def B(name, N, D, graphs, work="ws"):
    return dict(id=f"batched-{name}", entry="batched", N=N, D=D, graphs=list(graphs), work=work, names=[gid(s) for s in graphs])


def _ragged(count, top, seed):
    fams = ("rand", "traj", "chain", "pchain", "cycle", "loops", "twocomp", "rchain")
    ns = [int(v) for v in _rng("ragged", seed).randint(0, top, count)]
    return [g("empty") if n == 0 else g("single") if n == 1 else g(fams[k % len(fams)], max(n, 4), k % 3 == 0, seed)
            for k, n in enumerate(ns)]


HOP_DS = (1, 2, 5, 20, 32)
HOP_GRAPHS = (g("chain", 40, True), g("pchain", 40, True), g("chain", 33, True), g("golden:mid_node0"), g("golden:via_node0"),
              g("mid0", 21, True), g("traj", 120), g("traj", 50, True), g("rchain", 25, True), g("star0", 10, True))
N273 = (g("traj", 273), g("empty"), g("single"), g("rand", 15), g("rand", 16, True), g("rand", 17), g("traj", 33), g("rand", 272, True))
N601 = (g("golden:cycle600"), g("chain", 560, True), g("pchain", 560, True))
DIRTY_A = (g("traj", 280, False, 1), g("rand", 17), g("chain", 33, True))
DIRTY_B = (g("rand", 280, True), g("empty"), g("cycle", 40, True))

CASES = [
    # one workgroup per graph, M in LDS
    B("lds-N1", 1, 20, [g("single"), g("loop", 1, True), g("empty"), g("loop", 1)]),
    B("lds-N2", 2, 20, [g("noedge", 2), g("chain", 2, True), g("cycle", 2, True), g("loop", 1, True), g("empty"), g("golden:walk2")]),
    B("lds-N3", 3, 5, [g("golden:via_node0"), g("golden:chain3"), g("cycle", 3, True), g("star0", 3, True), g("complete", 3, True)]),
    B("lds-N9", 9, 20, [g("star0", 9, True), g("complete", 9, True), g("twocomp", 9, True), g("loops", 9), g("mid0", 9, True),
                        g("golden:mid_node0"), g("golden:components"), g("rchain", 9, True), g("golden:rand7"), g("noedge", 2)]),
    B("lds-N31", 31, 20, [g("rand", 31), g("traj", 31), g("pchain", 31, True), g("chain", 30, True), g("empty"), g("single")]),
    B("lds-N64-ragged", 64, 20, [g("traj", 64), g("rand", 64), g("chain", 64, True), g("pchain", 50, True), g("cycle", 33, True),
                                 g("twocomp", 17), g("empty")]),
    B("lds-N271", LDS_MAX_N - 1, 2, [g("traj", LDS_MAX_N - 1), g("rand", 40)]),
    B("lds-N272", LDS_MAX_N, 2, [g("traj", LDS_MAX_N), g("empty")]),
    # SPLIT_PARTS workgroups per graph
    B("split-N273", LDS_MAX_N + 1, 2, N273),
    B("split-N280-G35", 280, 2, [g("traj", 280)] + _ragged(34, 60, 3)),
    B("split-N1088-G17", SPLIT_MAX_N, 1, [g("rand", SPLIT_MAX_N - 7)] + _ragged(16, 41, 5)),
    B("split-N601", 601, 20, N601),
    B("split-dirty-a", 280, 5, DIRTY_A),
    B("split-dirty-b", 280, 5, DIRTY_B),
    # one workgroup per graph out of global memory
    B("global-N273", LDS_MAX_N + 1, 2, N273, work=None),
    B("global-N601", 601, 20, N601, work=None),
    B("global-N1089", SPLIT_MAX_N + 1, 2, [g("empty"), g("loop", 1, True), g("chain", 2, True), g("traj", 37), g("traj", 300)]),
    B("global-N1100", 1100, 2, [g("rand", 300, True), g("pchain", 37, True), g("noedge", 2), g("single"), g("empty")]),
    # hop counts and saturation
    *[B(f"hops-D{D}", 120, D, HOP_GRAPHS) for D in HOP_DS],
]
CASE = {c["id"]: c for c in CASES}


def check_coverage(cases=CASES):
    ids = [c["id"] for c in cases]
    assert len(set(ids)) == len(ids)
    by = {}
    for c in cases:
        by.setdefault(branch(c["N"], c["work"] is not None), []).append(c)
    assert set(by) == {"lds", "split", "global"}
    assert {c["N"] for c in by["lds"]} >= {1, 2, 3, 9, 31, 64, LDS_MAX_N - 1, LDS_MAX_N}
    assert {c["N"] for c in by["split"]} >= {LDS_MAX_N + 1, 280, 601, SPLIT_MAX_N}
    assert {c["N"] for c in by["global"]} >= {LDS_MAX_N + 1, 601, SPLIT_MAX_N + 1, 1100}
    assert (LDS_MAX_N, SPLIT_MAX_N, SPLIT_PARTS, MAX_D) == (272, 1088, 16, 32)
    ns = lambda cid: [graph(s).shape[0] for s in CASE[cid]["graphs"]]                        # noqa: E731
    assert sorted(ns("batched-split-N273")) == [0, 1, 15, 16, 17, 33, 272, 273] and (LDS_MAX_N + 1) % 2 == 1
    assert len(ns("batched-split-N280-G35")) == 35 and len(ns("batched-lds-N64-ragged")) == 7
    big = ns("batched-split-N1088-G17")
    assert len(big) == 17 and big[0] == 1081 and big[0] % 8 and max(big[1:]) <= 40
    assert ns("batched-lds-N272") == [LDS_MAX_N, 0]
    for cid in ("batched-global-N1089", "batched-global-N1100"):
        assert sorted(ns(cid)) == [0, 1, 2, 37, 300]
    for c in by["global"]:
        assert c["N"] <= SPLIT_MAX_N or max(ns(c["id"])) <= 320
    assert {c["D"] for c in cases} >= set(HOP_DS) and MAX_D in HOP_DS
    # split geometry: a workgroup without rows (n < SPLIT_PARTS), n odd, n % 8 != 0, n = N with N odd
    sp = [n for c in by["split"] for n in ns(c["id"])]
    assert any(0 < n < SPLIT_PARTS for n in sp) and any(n % 2 for n in sp) and any(n % 8 for n in sp) and 0 in sp


def hop_lengths(spec):
    """The set of hop counts of a graph's walks (what D is compared with)."""
    return {len(h) for h in prefix_hops(fw(spec)[1], 10 ** 6).values()}


# ------------------------------------------------------------------------------------------------ mobgt_collate_finish
RPMS = (0, 1, 3, 509, 510, 511, 1024)
SPD_VALUES = (-1, 0, 1, 2, 3, 508, 509, 510)
# beyond what mobgt_spd_batched writes: the header's sentence holds for any int16, and only such values tell whether the cut is
# really off above 510
SPD_VALUES_WIDE = SPD_VALUES + (511, 1023, 1024, 32767)
TABLES = ("null", "contig", "wide")
COLLATE_NS = (1, 2, 15, 33)
COLLATE_SHAPES = tuple(s for N in COLLATE_NS for s in ((1, N, (N,)), (1, N, (0,)), (3, N, (0, N, (N + 1) // 2)))) + ((1, 1030, (1030,)),)
TABLE_P = 37                                            # the table's last row id
NEG_INF_BITS, ZERO_BITS = -8388608, 0                   # float32 -inf and +0 as int32 patterns

_COLLATE = {}


def collate_inputs(G, N, n_nodes, wide_spd=False):
    """x, n_nodes, a synthetic spd and the [P + 1, P + 1] table whose row 0 and column 0 are non-zero (a lookup for x = 0 shows)."""
    key = (G, N, tuple(n_nodes), wide_spd)
    if key not in _COLLATE:
        rng = _rng("collate", *key)
        x = rng.randint(1, TABLE_P + 1, (G, N)).astype(np.int32)
        x[rng.rand(G, N) < 0.25] = 0                                            # zeros among the real nodes
        x.flat[rng.randint(0, G * N)] = TABLE_P
        if N >= 2:
            x[0, 0], x[0, 1] = 0, TABLE_P
        n_nodes = np.asarray(n_nodes, np.int32)
        assert n_nodes.shape == (G,)
        vals = np.asarray(SPD_VALUES_WIDE if wide_spd else SPD_VALUES, np.int16)
        spd = vals[rng.randint(0, vals.size, (G, N, N))]
        if N * N * G >= vals.size:
            spd.flat[rng.permutation(spd.size)[:vals.size]] = vals
        table = rng.randint(1, 64, (TABLE_P + 1, TABLE_P + 1)).astype(np.int16)
        _COLLATE[key] = dict(G=G, N=N, x=x, n_nodes=n_nodes, spd=spd, table=table)
    return _COLLATE[key]


def expected_collate(c, rel_pos_max, with_table, mut=None):
    """attn_bias [G, N + 1, N + 1] as int32 patterns and poi_pos [G, N, N] int16, from the header's sentence: 0 for key columns
    0 .. n_nodes[g] and -inf beyond; -inf where spd >= rel_pos_max when rel_pos_max <= 510; poi_pos = bin_table[x_i, x_j] where
    both are non-zero, else 0 (all 0 without a table)."""
    G, N, x, n, spd = c["G"], c["N"], c["x"].astype(np.int64), c["n_nodes"].astype(np.int64), c["spd"].astype(np.int64)
    T = N + 1
    cols = np.arange(T, dtype=np.int64)[None, None, :]
    last = n[:, None, None] + {"col_n_not_key": -1, "col_n1_key": 1}.get(mut, 0)
    ab = np.where(np.broadcast_to(cols, (G, T, T)) <= last, ZERO_BITS, NEG_INF_BITS).astype(np.int32)
    if rel_pos_max <= 510 or mut == "cut_above_510":
        far = spd > rel_pos_max if mut == "cut_gt" else spd >= rel_pos_max
        ab[:, 1:, 1:][far] = NEG_INF_BITS
    pp = np.zeros((G, N, N), np.int16)
    if with_table:
        xi, xj = np.broadcast_to(x[:, :, None], (G, N, N)), np.broadcast_to(x[:, None, :], (G, N, N))
        looked = c["table"][xi, xj]
        pp = looked if mut == "poi_pos_x0" else np.where((xi != 0) & (xj != 0), looked, 0).astype(np.int16)
    return dict(attn_bias=ab, poi_pos=pp)


# ------------------------------------------------------------------------------------------------ the single-graph entries
FW_NS = (1, 2, 5, LDS_MAX_N, LDS_MAX_N + 1, 300)
FEATURE_VALUES = (2 ** 24 + 1, -7, 2 ** 40 + 1, 0, 1, 3)


def fw_spec(n):
    return g("traj" if n > 2 else "chain", n)


def edge_feat(n, F, seed=0):
    """int64 [n, n, F] holding values that do not survive the float64 -> float32 trip."""
    rng = _rng("feat", n, F, seed)
    f = np.asarray(FEATURE_VALUES, np.int64)[rng.randint(0, len(FEATURE_VALUES), (n, n, F))]
    f.flat[:len(FEATURE_VALUES)] = FEATURE_VALUES
    return f


GEN_GRAPHS = (g("chain", 7), g("golden:mid_node0"), g("golden:rand7"), g("pchain", 12))


def longest_path(spec):
    return max(hop_lengths(spec))


def malformed():
    """Path matrices that are no Floyd-Warshall output, every entry in [0, n): {name: (path, err_flag of mobgt_gen_edge_input at
    max_dist = 4, a pair (i, j) whose walk never ends)}.
        two_cycle   0 -> 2 goes through 1 and 0 -> 1 through 2: the stack only grows               -> 2 (deeper than any valid path)
        identity    path[i][j] = j: the target is pushed again and again                            -> 2
        leafy_loop  1 and 2 hand the target 3 to each other, one emitted hop per turn                -> 1 (more hops than max_dist)
    Code 3 (the iteration guard) cannot be reached: a walk that has not reported 1 has emitted at most max_dist hops, its pushes
    are at most its pops + cap - 1, so it ends within 2 max_dist + cap < 4 n + 2 max_dist + 8 iterations."""
    two = np.zeros((3, 3), np.int64)
    two[0, 2], two[0, 1] = 1, 2
    ident = np.tile(np.arange(4, dtype=np.int64), (4, 1))
    leafy = np.zeros((4, 4), np.int64)
    leafy[0, 3], leafy[1, 3], leafy[2, 3] = 1, 2, 1
    return dict(two_cycle=(two, 2, (0, 2)), identity=(ident, 2, (0, 1)), leafy_loop=(leafy, 1, (0, 3)))
