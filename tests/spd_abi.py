"""The shortest-path preprocessing's C ABI (include/mobgt_hip.h: mobgt_spd_workspace_bytes / mobgt_spd_batched /
mobgt_spd_set_spin_limit / mobgt_collate_finish / mobgt_floyd_warshall_workspace_bytes / mobgt_floyd_warshall /
mobgt_gen_edge_input / mobgt_get_all_edges of csrc/spd.hip) as plain Python callers over device pointers.  Every size is an
argument; an operand may be a tensor, a GuardedFlat, a raw address or None (`work`, `bin_table`).  Every caller RETURNS the status
code (0 = launched)."""
from mobgt_amd import _lib
from mobgt_amd.ops import _stream

C = _lib.CONSTANTS
EBADDIM = C["MOBGT_EBADDIM"]
LDS_MAX_N, SPLIT_MAX_N, SPLIT_PARTS, MAX_D = (C["MOBGT_SPD_" + n] for n in ("LDS_MAX_N", "SPLIT_MAX_N", "SPLIT_PARTS", "MAX_D"))


def addr(t):
    if t is None or isinstance(t, int):
        return t
    return t.ptr() if hasattr(t, "ptr") else t.data_ptr()


def spd_workspace_bytes(G, N):
    return int(_lib.lib().mobgt_spd_workspace_bytes(G, N))


def spd_batched(counts, n_nodes, spd, path, rel_pos, edge_input, in_degree, out_degree, work, G, N, D):
    return _lib.lib().mobgt_spd_batched(addr(counts), addr(n_nodes), addr(spd), addr(path), addr(rel_pos), addr(edge_input),
                                        addr(in_degree), addr(out_degree), addr(work), G, N, D, _stream())


def spd_set_spin_limit(ticks):
    return _lib.lib().mobgt_spd_set_spin_limit(int(ticks))


def collate_finish(x, n_nodes, spd, bin_table, ld_bin, rel_pos_max, attn_bias, poi_pos, G, N):
    return _lib.lib().mobgt_collate_finish(addr(x), addr(n_nodes), addr(spd), addr(bin_table), int(ld_bin), int(rel_pos_max),
                                           addr(attn_bias), addr(poi_pos), G, N, _stream())


def floyd_warshall_workspace_bytes(n):
    return int(_lib.lib().mobgt_floyd_warshall_workspace_bytes(n))


def floyd_warshall(adj, n, M, path, work):
    return _lib.lib().mobgt_floyd_warshall(addr(adj), n, addr(M), addr(path), addr(work), _stream())


def gen_edge_input(max_dist, path, edge_feat, n, F, out, err_flag):
    return _lib.lib().mobgt_gen_edge_input(int(max_dist), addr(path), addr(edge_feat), n, F, addr(out), addr(err_flag), _stream())


def get_all_edges(path, n, i, j, out_nodes, out_len, work):
    return _lib.lib().mobgt_get_all_edges(addr(path), n, int(i), int(j), addr(out_nodes), addr(out_len), addr(work), _stream())
