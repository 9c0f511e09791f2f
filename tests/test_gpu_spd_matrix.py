"""The shortest-path preprocessing kernels (csrc/spd.hip) through every entry point of their C ABI, against the expected outputs
that tests/spd_reference.py derives from the committed oracle.  Everything is integer data (attn_bias: bit patterns), compared
with np.array_equal over the whole array, padding included -- there is no tolerance anywhere.

Every output is a view inside a poison-filled buffer (int16 -12345, uint8 0xA5, a NaN pattern for floats) with guard elements on
either side that must stay untouched; the workspaces are exactly as long as the *_workspace_bytes functions say, with a guard
behind them.  The padding rows and columns of `counts` hold a non-zero count, which the contract says is ignored.  The Floyd-
Warshall branch of every batched case (one workgroup in LDS, several workgroups per graph, one workgroup out of global memory) is
decided from the thresholds the header declares; the boundary shapes are named from the same constants.
tests/test_host_spd_reference.py shows on the CPU that the verdicts reject the defects they are meant to reject."""
import numpy as np
import pytest
import torch

import spd_abi as abi
import spd_reference as sr
from matrix_helpers import DEV, GuardedFlat, dev
from oracle import algos_oracle as ao

pytestmark = pytest.mark.gpu
I16, U8, I32, I64, F32 = torch.int16, torch.uint8, torch.int32, torch.int64, torch.float32


class Outputs:
    """The six destinations of mobgt_spd_batched for (G, N, D), in the order of its arguments."""

    def __init__(self, G, N, D):
        shapes = dict(spd=((G, N, N), I16), path=((G, N, N), I16), rel_pos=((G, N, N), I16), edge_input=((G, N, N, D), U8),
                      in_degree=((G, N), I16), out_degree=((G, N), I16))
        self.bufs = {k: GuardedFlat(s, t) for k, (s, t) in shapes.items()}

    def views(self):
        return [self.bufs[k] for k in sr.FIELDS]

    def results(self):
        return {k: b.result() for k, b in self.bufs.items()}

    def untouched(self):
        return all(b.untouched() for b in self.bufs.values())


def workspace(nbytes, fill=None):
    """`nbytes` of scratch with a guard behind it (and in front); fill: the byte the scratch starts as (default: the poison)."""
    return GuardedFlat((nbytes,), U8, guard=256, init=None if fill is None else np.full(nbytes, fill, np.uint8))


def run_batched(case, ws=None):
    """One call of a batched case (ws: a workspace to reuse); every field against the reference, every guard intact."""
    G, N, D = len(case["graphs"]), case["N"], case["D"]
    counts, n_nodes = sr.batch_inputs(case)
    want = sr.expected_batched(case)
    cd, nd = dev(counts), dev(n_nodes)
    outs = Outputs(G, N, D)
    if case["work"] is not None and ws is None:
        ws = workspace(abi.spd_workspace_bytes(G, N))
    assert abi.spd_batched(cd, nd, *outs.views(), ws if case["work"] is not None else None, G, N, D) == 0
    torch.cuda.synchronize()
    got = outs.results()
    gave_up = None
    if ws is not None and sr.branch(N, True) == "split":
        gave_up = ws.result()[:(G * N + G) * 4].view(np.int32)[G * N:]           # one flag per graph: handed to the redo pass
        print(f"spd-redone {case['id']} {int((gave_up != 0).sum())} of {G}")
    ok, msg = sr.judge(want, got, case["names"])
    assert ok, (case["id"], msg)
    return gave_up


@pytest.mark.parametrize("case", sr.CASES, ids=lambda c: f"{c['id']}-{sr.branch(c['N'], c['work'] is not None)}")
def test_batched(case):
    kind = case["id"].split("-")[1]
    assert sr.branch(case["N"], case["work"] is not None) == dict(hops="lds").get(kind, kind)
    run_batched(case)


def test_workspace_sizes():
    for G, N in ((1, 1), (3, sr.LDS_MAX_N), (1, sr.SPLIT_MAX_N + 1), (0, 500), (4, 32000)):
        assert abi.spd_workspace_bytes(G, N) == 16
    for G, N in ((1, sr.LDS_MAX_N + 1), (35, 280), (17, sr.SPLIT_MAX_N)):
        npw = ((N + 7) & ~7) // 2
        assert abi.spd_workspace_bytes(G, N) == (G * N + G) * 4 + G * N * npw * 4 + 16


def test_a_dirty_workspace_is_reused():
    """Two different batches, then the first again, through one workspace that starts as 0xFF and is never cleared between them."""
    a, b = sr.CASE["batched-split-dirty-a"], sr.CASE["batched-split-dirty-b"]
    assert (len(a["graphs"]), a["N"]) == (len(b["graphs"]), b["N"])
    ws = workspace(abi.spd_workspace_bytes(len(a["graphs"]), a["N"]), fill=0xFF)
    for case in (a, b, a):
        run_batched(case, ws)


def test_redo_pass_under_a_zero_wait_bound():
    """Every waiter gives up at once: the single-workgroup redo pass must deliver the same arrays."""
    case = sr.CASE["batched-split-N273"]
    try:
        assert abi.spd_set_spin_limit(0) == 0
        gave_up = run_batched(case)
    finally:
        assert abi.spd_set_spin_limit(-1) == 0
    n = np.asarray([sr.graph(s).shape[0] for s in case["graphs"]])
    # which graphs went through the redo pass is a matter of timing (a waiter that finds its row already published goes on) and is
    # printed, not asserted; a graph with one workgroup that has rows waits for nobody
    assert set(np.unique(gave_up)) <= {0, 1} and not gave_up[n <= 1].any()
    run_batched(case)


REFUSED = {"D-1": dict(D=-1), "D0": dict(D=0), "D33": dict(D=sr.MAX_D + 1), "G0": dict(G=0), "N0": dict(N=0), "G-1": dict(G=-1)}


@pytest.mark.parametrize("name", list(REFUSED), ids=list(REFUSED))
def test_batched_refusal_writes_nothing(name):
    case = sr.CASE["batched-lds-N9"]
    counts, n_nodes = sr.batch_inputs(case)
    a = dict(G=len(case["graphs"]), N=case["N"], D=case["D"])
    outs = Outputs(a["G"], a["N"], sr.MAX_D + 1)
    ws = workspace(16)
    a.update(REFUSED[name])
    assert abi.spd_batched(dev(counts), dev(n_nodes), *outs.views(), ws, a["G"], a["N"], a["D"]) == abi.EBADDIM
    torch.cuda.synchronize()
    assert outs.untouched() and ws.untouched()


def test_batched_refusal_of_n_32001_reads_no_pointer():
    tiny = [GuardedFlat((16,), U8) for _ in range(9)]
    assert abi.spd_batched(*tiny, 1, 32001, 20) == abi.EBADDIM
    torch.cuda.synchronize()
    assert all(t.untouched() for t in tiny)


# ------------------------------------------------------------------------------------------------ mobgt_collate_finish
def _table(c, mode):
    """(operand, ld_bin): None; the contiguous table; the table as columns 3 .. 3 + P of a wider buffer of 1000s."""
    if mode == "null":
        return None, 0
    if mode == "contig":
        return dev(c["table"]), c["table"].shape[1]
    wide = torch.full((c["table"].shape[0], c["table"].shape[1] + 8), 1000, dtype=I16, device=DEV)
    v = wide[:, 3:3 + c["table"].shape[1]]
    v.copy_(dev(c["table"]))
    return v, wide.shape[1]


@pytest.mark.parametrize("mode", sr.TABLES)
@pytest.mark.parametrize("shape", sr.COLLATE_SHAPES, ids=lambda s: f"G{s[0]}-N{s[1]}-n{'_'.join(map(str, s[2]))}")
def test_collate_finish(shape, mode):
    G, N, nn = shape
    for wide_spd in (False, True):
        c = sr.collate_inputs(G, N, nn, wide_spd)
        x, nd, spd = dev(c["x"]), dev(c["n_nodes"]), dev(c["spd"])
        table, ld = _table(c, mode)
        for rpm in sr.RPMS:
            ab, pp = GuardedFlat((G, N + 1, N + 1), F32), GuardedFlat((G, N, N), I16)
            assert abi.collate_finish(x, nd, spd, table, ld, rpm, ab, pp, G, N) == 0
            torch.cuda.synchronize()
            ok, msg = sr.judge(sr.expected_collate(c, rpm, mode != "null"), dict(attn_bias=ab.result(), poi_pos=pp.result()))
            assert ok, (shape, mode, wide_spd, rpm, msg)


@pytest.mark.parametrize("G,N", [(0, 5), (2, 0), (-1, 5)])
def test_collate_finish_refusal_writes_nothing(G, N):
    c = sr.collate_inputs(3, 15, (0, 15, 8))
    ab, pp = GuardedFlat((3, 16, 16), F32), GuardedFlat((3, 15, 15), I16)
    assert abi.collate_finish(dev(c["x"]), dev(c["n_nodes"]), dev(c["spd"]), None, 0, 20, ab, pp, G, N) == abi.EBADDIM
    torch.cuda.synchronize()
    assert ab.untouched() and pp.untouched()


# ------------------------------------------------------------------------------------------------ the single-graph entries
@pytest.mark.parametrize("n", sr.FW_NS)
def test_floyd_warshall(n):
    spec = sr.fw_spec(n)
    M, P = GuardedFlat((n, n), I64), GuardedFlat((n, n), I64)
    ws = workspace(abi.floyd_warshall_workspace_bytes(n))
    assert abi.floyd_warshall(dev(np.array(sr.graph(spec))), n, M, P, ws) == 0   # (the counts themselves: non-zero = edge)
    torch.cuda.synchronize()
    ws.result()
    ok, msg = sr.judge(dict(zip(("M", "path"), sr.fw(spec))), dict(M=M.result(), path=P.result()))
    assert ok, (n, msg)


def _gen(max_dist, path, feat):
    """(status, err_flag, out as int32 patterns) of one mobgt_gen_edge_input call; guards checked."""
    n, F = path.shape[0], feat.shape[-1]
    out, err = GuardedFlat((n, n, max_dist, F), F32), GuardedFlat((1,), I32)
    st = abi.gen_edge_input(max_dist, dev(path), dev(feat), n, F, out, err)
    torch.cuda.synchronize()
    return st, int(err.result()[0]), out.result()


@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("spec", sr.GEN_GRAPHS, ids=sr.gid)
def test_gen_edge_input(spec, F, monkeypatch):
    """max_dist 0, 1, the longest walk (the deepest legal stack) and one below it; features that do not survive the float64 ->
    float32 trip.  Where a walk is longer than max_dist the flag is 1 or 2 and the drop-in raises IndexError, as the reference's
    bounds check does -- max_dist = 0 included."""
    from mobgt_amd import algos
    monkeypatch.setenv("MOBGT_ALGOS_BACKEND", "device")
    P = sr.fw(spec)[1]
    n = P.shape[0]
    feat = sr.edge_feat(n, F)
    L = sr.longest_path(spec)
    for md in (0, 1, L, L - 1):
        st, err, out = _gen(md, P, feat)
        assert st == 0
        if md >= L:
            want = sr.first_hops(P, feat, md)
            assert err == 0 and np.array_equal(out, want.view(np.int32)), (sr.gid(spec), md)
            assert np.array_equal(algos.gen_edge_input(md, P, feat), want)
            assert np.array_equal(want, ao.gen_edge_input(md, P, feat))
        else:
            assert err in (1, 2), (sr.gid(spec), md, err)
            with pytest.raises(IndexError):
                ao.gen_edge_input(md, P, feat)
            with pytest.raises(IndexError):
                algos.gen_edge_input(md, P, feat)


def test_gen_edge_input_without_a_walk_and_refusals():
    one = np.zeros((1, 1), np.int64)
    for md in (0, 3):
        st, err, out = _gen(md, one, np.full((1, 1, 2), 9, np.int64))
        assert (st, err) == (0, 0) and (out.view(np.float32) == -1).all()
    P = sr.fw(sr.GEN_GRAPHS[0])[1]
    n = P.shape[0]
    for kw in (dict(n=0), dict(F=0), dict(max_dist=-1)):
        a = dict(n=n, F=1, max_dist=3)
        a.update(kw)
        out, err = GuardedFlat((n, n, 3, 1), F32), GuardedFlat((1,), I32)
        assert abi.gen_edge_input(a["max_dist"], dev(P), dev(sr.edge_feat(n, 1)), a["n"], a["F"], out, err) == abi.EBADDIM
        torch.cuda.synchronize()
        assert out.untouched() and err.untouched()


@pytest.mark.parametrize("name", list(sr.malformed()))
def test_malformed_path_matrices(name):
    """Path matrices that are no Floyd-Warshall output (every entry inside [0, n)): the flag of mobgt_gen_edge_input and the -1 of
    mobgt_get_all_edges.  See spd_reference.malformed for why the flag is never 3."""
    path, code, (i, j) = sr.malformed()[name]
    n = path.shape[0]
    st, err, _ = _gen(4, path, sr.edge_feat(n, 1))
    assert (st, err) == (0, code)
    out, ln, work = GuardedFlat((n + 2,), I32), GuardedFlat((1,), I32), GuardedFlat((2 * n + 4,), I32)
    assert abi.get_all_edges(dev(path), n, i, j, out, ln, work) == 0
    torch.cuda.synchronize()
    out.result(), work.result()
    assert ln.result()[0] == -1


def test_get_all_edges_on_every_pair_of_the_small_golden_graphs():
    for name in sr.golden_names():
        spec = sr.g("golden:" + name)
        P = sr.fw(spec)[1]
        n = P.shape[0]
        if n > 7:
            continue
        pairs = [(i, j) for i in range(n) for j in range(n) if P[i, j] != sr.UNREACH]      # (510 is no index into a 7 x 7 matrix)
        out, ln, work = GuardedFlat((len(pairs), n + 2), I32), GuardedFlat((len(pairs),), I32), GuardedFlat((2 * n + 4,), I32)
        pd = dev(P)
        for k, (i, j) in enumerate(pairs):
            assert abi.get_all_edges(pd, n, i, j, out.ptr() + 4 * k * (n + 2), ln.ptr() + 4 * k, work) == 0
        torch.cuda.synchronize()
        nodes, lens = out.result(), ln.result()
        work.result()
        for k, (i, j) in enumerate(pairs):
            want = ao.get_all_edges(P, i, j)
            assert lens[k] == len(want) and list(nodes[k, :len(want)]) == want, (name, i, j)
            assert (nodes[k, len(want):] == out.poison).all(), (name, i, j)
    P = sr.fw(sr.g("golden:chain5"))[1]
    out, ln, work = GuardedFlat((7,), I32), GuardedFlat((1,), I32), GuardedFlat((14,), I32)
    for n, i, j in ((0, 0, 0), (5, -1, 0), (5, 0, 5), (5, 5, 0), (5, 0, -1)):
        assert abi.get_all_edges(dev(P), n, i, j, out, ln, work) == abi.EBADDIM
    torch.cuda.synchronize()
    assert out.untouched() and ln.untouched() and work.untouched()
