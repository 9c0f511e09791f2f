"""CPU checks of the shortest-path matrix's reference side (tests/spd_reference.py): it reproduces the reference's own outputs
(golden G1), the oracle's tolerant "first D hops" call equals a restatement that shares no algorithm with the kernel (and the
kernel's bounded ring equals both, which is the header's claim), the case list reaches every dispatch branch and boundary, every
wrong reference (MUTANTS) is rejected by a case the GPU matrix runs, and the whole set of references is quick to compute."""
import time

import numpy as np
import pytest

import spd_reference as sr
from oracle import algos_oracle as ao

SMALL = sorted({s for c in sr.CASES for s in c["graphs"] if sr.graph(s).shape[0] <= 64}, key=sr.gid)


def test_the_matrix_reaches_every_branch_boundary_and_hop_count():
    sr.check_coverage()
    assert (sr.branch(272, True), sr.branch(273, True), sr.branch(273, False)) == ("lds", "split", "global")
    assert (sr.branch(1088, True), sr.branch(1089, True), sr.branch(1088, False)) == ("split", "global", "global")
    fams = {s[0].split(":")[0] for c in sr.CASES for s in c["graphs"]}
    assert fams >= set(sr.FAMILIES) | {"golden"}
    used = {int(v) for c in sr.CASES for s in c["graphs"] if s[2] for v in np.unique(sr.graph(s))} - {0}
    assert used == set(sr.SAT_COUNTS)
    # the hop cases hold walks shorter than, exactly as long as and longer than every D; saturating counts lie on their walks
    lengths = set().union(*[sr.hop_lengths(s) for s in sr.HOP_GRAPHS])
    for D in sr.HOP_DS:
        assert {D - 1, D, D + 1} - {0} <= lengths, D
    e = sr.expected_batched(sr.CASE["batched-hops-D32"])["edge_input"]
    assert {int(v) for v in np.unique(e)} >= {0, 1, 4, 5, 252, 253, 254, 255}
    # the node-0 quirk shows: a hop over a non-edge
    assert (sr.expected_batched(sr.CASE["batched-lds-N9"])["edge_input"] == 1).any()


def test_the_reference_reproduces_golden_g1():
    for name in sr.golden_names():
        z = sr.golden(name)
        spec = sr.g("golden:" + name)
        M, P = sr.fw(spec)
        assert np.array_equal(M, z["M"]) and np.array_equal(P, z["path"]), name
        if "edge_input20" not in z:
            assert name == "cycle600"
            continue
        c = sr.graph(spec)
        feat = np.where(c != 0, c + 2, 0)[:, :, None]
        want = z["edge_input20"]
        got = sr.first_hops(P, feat, 20)
        assert np.array_equal(got[:, :, :want.shape[2]], want) and (got[:, :, want.shape[2]:] == -1).all(), name
        if c.max(initial=0) <= 252:                     # the batched layout: the reference's feature + 1, -1 -> 0
            e = sr.graph_outputs(spec, 20)["hops"]
            assert np.array_equal(e[:, :, :want.shape[2]].astype(np.int64), want[..., 0].astype(np.int64) + 1), name


@pytest.mark.parametrize("D", [1, 2, 5, 20, 32])
def test_restatement_equals_the_tolerant_oracle_call(D):
    """The memoised-prefix restatement against oracle_gen_edge_input at max_dist = D on every graph of the matrix with n <= 64 --
    and the kernel's ring of D pending targets (oldest overwritten) against both on the graphs of at most 40 nodes."""
    assert len(SMALL) > 40
    for spec in SMALL:
        c = sr.graph(spec)
        n = c.shape[0]
        M, P = sr.fw(spec)
        feat = sr.feature(c)
        want = sr.graph_outputs(spec, D)["hops"]
        hops = sr.prefix_hops(P, D)
        assert np.array_equal(sr.hops_array(hops, feat, n, D), want), sr.gid(spec)
        if n <= 40:
            assert sr.lifo_hops(P, D) == hops, sr.gid(spec)
        # the hop endpoints themselves, through a feature that names the pair
        pair = (np.arange(n)[:, None] * n + np.arange(n)[None, :] + 1)[:, :, None]
        ids = sr.first_hops(P, pair, D)[..., 0]
        for (i, j), hs in hops.items():
            assert [a * n + b + 1 for a, b in hs] == [int(v) for v in ids[i, j, :len(hs)]] and (ids[i, j, len(hs):] == -1).all()
        walked = np.zeros((n, n), bool)
        for i, j in hops:
            walked[i, j] = True
        assert (ids[~walked] == -1).all()


def test_numpy_floyd_warshall_of_the_mutants_is_the_oracle_when_unmutated():
    for spec in SMALL:
        M, P = sr.np_fw(sr.graph(spec) != 0)
        assert np.array_equal(M, sr.fw(spec)[0]) and np.array_equal(P, sr.fw(spec)[1]), sr.gid(spec)


def test_full_path_of_the_long_graphs_by_hand():
    """The literal-510 region: in a graph of more than 510 nodes a pair whose path entry is the NODE 510 reads as unreachable at
    the top level and is still walked through as a sub-path.  The tolerant call against ao.get_all_edges on such pairs."""
    seen = 0
    for spec in sr.N601[1:]:
        M, P = sr.fw(spec)
        n = P.shape[0]
        c = sr.graph(spec)
        lit = np.argwhere((P == sr.UNREACH) & (M < sr.UNREACH))
        assert len(lit) > 0, sr.gid(spec)
        e = sr.graph_outputs(spec, 20)["hops"]
        assert (e[lit[:, 0], lit[:, 1]] == 0).all()                             # read as unreachable at the top level
        via = np.argwhere((M < sr.UNREACH) & (M > 1) & (P != sr.UNREACH))
        rng = np.random.RandomState(3)
        feat = sr.feature(c)
        for i, j in via[rng.permutation(len(via))[:300]]:
            nodes = [int(i)] + ao.get_all_edges(P, i, j) + [int(j)]
            seen += sr.UNREACH in nodes[1:-1]
            want = [feat[a, b] for a, b in zip(nodes[:-1], nodes[1:])][:20]
            assert list(e[i, j, :len(want)]) == want and (e[i, j, len(want):] == 0).all(), (sr.gid(spec), i, j)
    assert seen > 0                                     # some compared walks pass through node 510 itself


@pytest.mark.parametrize("mut", sr.FW_MUTANTS + sr.HOP_MUTANTS + sr.PAD_MUTANTS)
def test_every_batched_mutant_is_rejected(mut):
    """At least one case of the matrix tells the wrong reference from the right one (the small cases first: the emulation of a
    wrong kernel is plain Python)."""
    rejected = []
    for case in sorted(sr.CASES, key=lambda c: c["N"] * c["N"] * len(c["graphs"])):
        if case["N"] > 120:
            break
        want = sr.expected_batched(case)
        assert sr.judge(want, want, case["names"])[0]
        ok, msg = sr.judge(want, sr.expected_batched(case, mut), case["names"])
        if not ok:
            rejected.append((case["id"], msg))
            if len(rejected) == 2:
                break
    print(mut, rejected)
    assert rejected, mut


@pytest.mark.parametrize("mut", sr.COLLATE_MUTANTS)
def test_every_collate_mutant_is_rejected(mut):
    rejected = []
    for G, N, nn in sr.COLLATE_SHAPES:
        if N > 33:
            continue
        for wide in (False, True):
            c = sr.collate_inputs(G, N, nn, wide)
            for rpm in sr.RPMS:
                want = sr.expected_collate(c, rpm, True)
                assert sr.judge(want, want)[0]
                if not sr.judge(want, sr.expected_collate(c, rpm, True, mut))[0]:
                    rejected.append((G, N, nn, wide, rpm))
    print(mut, rejected[:4])
    assert rejected, mut
    if mut == "cut_above_510":                          # only spd values mobgt_spd_batched never writes can tell
        assert all(r[3] and r[4] > 510 for r in rejected)


def test_collate_reference_is_the_plain_loop():
    for G, N, nn in ((3, 15, (0, 15, 8)), (1, 2, (2,))):
        c = sr.collate_inputs(G, N, nn, True)
        for rpm in sr.RPMS:
            e = sr.expected_collate(c, rpm, True)
            ab = e["attn_bias"].view(np.float32)
            for gg in range(G):
                for i in range(N + 1):
                    for j in range(N + 1):
                        w = 0.0 if j <= c["n_nodes"][gg] else -np.inf
                        if i and j and rpm <= 510 and c["spd"][gg, i - 1, j - 1] >= rpm:
                            w = -np.inf
                        assert ab[gg, i, j] == w
                        if i and j:
                            xi, xj = c["x"][gg, i - 1], c["x"][gg, j - 1]
                            assert e["poi_pos"][gg, i - 1, j - 1] == (c["table"][xi, xj] if xi and xj else 0)
            assert not sr.expected_collate(c, rpm, False)["poi_pos"].any()
    c = sr.collate_inputs(3, 33, (0, 33, 17), False)
    assert set(np.unique(c["spd"])) == set(sr.SPD_VALUES) and (c["x"] == 0).any() and (c["x"] == sr.TABLE_P).any()
    assert (c["table"][0] != 0).all() and (c["table"][:, 0] != 0).all()


def test_single_graph_entry_references():
    # the float64 -> float32 trip of the features
    f = sr.edge_feat(7, 3)
    assert {int(v) for v in np.unique(f)} == set(sr.FEATURE_VALUES)
    assert np.float32(np.float64(2 ** 24 + 1)) == 2 ** 24 and np.float32(np.float64(2 ** 40 + 1)) == 2 ** 40
    for spec in sr.GEN_GRAPHS:
        M, P = sr.fw(spec)
        L = sr.longest_path(spec)
        assert 1 < L <= int(M[M < sr.UNREACH].max())    # (a walk through node 0 has fewer hops than its distance)
        n = P.shape[0]
        full = ao.gen_edge_input(L, P, sr.edge_feat(n, 3))                      # no IndexError at the longest walk
        assert np.array_equal(full, sr.first_hops(P, sr.edge_feat(n, 3), L))
        assert {float(v) for v in np.unique(full)} <= {-1.0} | {float(np.float32(np.float64(v))) for v in sr.FEATURE_VALUES}
        if L > 1:
            with pytest.raises(IndexError):
                ao.gen_edge_input(L - 1, P, sr.edge_feat(n, 3))
    # the malformed matrices: every entry inside [0, n), and the oracle's walk does not end either
    for name, (path, code, (i, j)) in sr.malformed().items():
        assert path.min() >= 0 and path.max() < path.shape[0] and code in (1, 2), name
        with pytest.raises(RecursionError):
            ao.get_all_edges(path, i, j)


def test_all_references_compute_in_under_a_minute():
    """Every reference of the GPU matrix, from cold caches."""
    for cache in (sr._FW, sr._PARTS, sr._EXPECTED):
        cache.clear()
    t0 = time.perf_counter()
    for case in sr.CASES:
        sr.batch_inputs(case)
        sr.expected_batched(case)
    for n in sr.FW_NS:
        sr.fw(sr.fw_spec(n))
    dt = time.perf_counter() - t0
    print(f"spd-reference-seconds {dt:.1f}")
    assert dt < 60.0
