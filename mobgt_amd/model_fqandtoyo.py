"""Drop-in counterpart of `graphormer/model_fqandtoyo.py` -- the Graphormer `entry.py:10` actually
runs -- for the `foursquaregraph` and `gowalla_*` datasets, on MI355X.

State-dict names and shapes equal the reference's (checked against the golden parameter list in
tests/golden/g6_e2e.npz), including the parameters the reference defines but never uses in `forward`
(`time_encoder`, `atom_encoder`, `poi_embed_model`, `fuse_embed`, `cat_embed_model`,
`embed_fuse_model1`, every `self_attention_norm`).

Differences in HOW (never in WHAT):
* bias assembly + multi-hop edge reduce, the attention core and the node-feature gathers are HIP kernels
  (`mobgt_amd.ops`);
* the reference's per-sample Python loops (model_fqandtoyo.py:1257-1269, 1353-1358) become batched
  gathers and two small GEMMs over all nodes; padded positions are masked to zero afterwards, as the
  reference leaves them;
* `embed_fuse_model3` / `final_ln` / ELU are evaluated for the graph token only -- the reference computes
  them for tokens 0..N-1 but reads `[:, 0, :]` alone (model_fqandtoyo.py:1394-1396), so the other rows
  never reach an output or a gradient.
"""
import os
import pickle

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import forms, ops
from .restriction import Restriction
from .step_state import STEP
from .lr import PolynomialDecayLR
from .model import (FeedForwardNetwork, MultiHeadAttention, hop_table_from, no_grad_row0, fused_layer_forward,
                    refresh_shadows, flush_pending_pack)
from .modelGNN import GCN, prelaunch_small_gcn

node_dim = 2000          # model_fqandtoyo.py:567


def freedman_diaconis_bins(x, return_bins=False):
    """model_fqandtoyo.py:570-577 / collator.py:301-308 (len(x) = rows of the matrix)."""
    iqr = np.subtract(*np.percentile(x, [75, 25]))
    binsize = 2 * iqr * np.power(len(x), -1 / 3)
    bins = np.ceil((np.max(x) - np.min(x)) / binsize)
    if return_bins:
        return int(bins), np.histogram(x, int(bins))[1]
    return int(bins)


def calculate_laplacian_matrix(adj_mat, mat_type="hat_rw_normd_lap_mat"):
    """model_fqandtoyo.py:456-486: (D+I)^-1 (A+I) with row-sum degrees (the only type the model uses)."""
    if mat_type != "hat_rw_normd_lap_mat":
        raise ValueError(f"ERROR: {mat_type} is unknown.")
    adj = np.asarray(adj_mat, dtype=np.float64)
    n = adj.shape[0]
    deg = np.sum(adj, axis=1) + 1.0
    return (adj + np.identity(n)) / deg[:, None]


def GradientTailLoss(inputs, targets, alpha=0.25, beta=1, k=1):
    """model_fqandtoyo.py:545-550 (device taken from `inputs` instead of the hard-coded "cuda")."""
    one_hot = torch.zeros_like(inputs)
    one_hot.scatter_(1, targets[:len(inputs)].view(-1, 1), 1)
    prob = torch.sigmoid(inputs)
    loss = -alpha * (1 - prob) ** k * one_hot * torch.log(prob) - (1 - one_hot) * beta * prob ** k * torch.log(1 - prob)
    return loss.mean()


class UserEmbeddings(nn.Module):
    def __init__(self, num_users, embedding_dim):
        super().__init__()
        self.user_embedding = nn.Embedding(num_embeddings=num_users, embedding_dim=embedding_dim)

    def forward(self, user_idx):
        return self.user_embedding(user_idx)


class CategoryEmbeddings(nn.Module):
    def __init__(self, num_cats, embedding_dim, padding_idx=0):
        super().__init__()
        self.cat_embedding = nn.Embedding(num_embeddings=num_cats, embedding_dim=embedding_dim, padding_idx=padding_idx)

    def forward(self, cat_idx):
        return self.cat_embedding(cat_idx)


class FuseEmbeddings(nn.Module):
    """model_fqandtoyo.py:440-455"""

    def __init__(self, user_embed_dim, poi_embed_dim):
        super().__init__()
        embed_dim = user_embed_dim + poi_embed_dim
        self.fuse_embed = nn.Linear(embed_dim, embed_dim)
        self.leaky_relu = nn.LeakyReLU(0.2)

    def forward(self, user_embed, poi_embed):
        x = torch.cat((user_embed, poi_embed), user_embed.dim() - 1)
        if x.is_cuda:           # Linear + LeakyReLU in one launch (the activation rides in the GEMM's epilogue)
            return ops.linear_splitk(x.float(), self.fuse_embed.weight, self.fuse_embed.bias, getattr(self, "bf16_wgrad", False),
                                     slope=self.leaky_relu.negative_slope)
        return self.leaky_relu(self.fuse_embed(x))


class LearnablePositionalEncoding(nn.Module):
    """model_fqandtoyo.py:328-358; only the parameter lives here, the adds are fused into the gathers."""

    def __init__(self, d_model, max_len, dropout=0.1):
        super().__init__()
        self.dropout = nn.Dropout(p=dropout)
        self.pe = nn.Parameter(torch.empty(d_model, max_len))
        nn.init.uniform_(self.pe, -0.02, 0.02)


class EncoderLayer(nn.Module):
    """model_fqandtoyo.py:1714-1743: attention WITHOUT pre-norm, LN1 before the FFN, LN2 on the output
    (`self_attention_norm` exists for checkpoint compatibility and is unused, as in the reference)."""

    def __init__(self, hidden_size, ffn_size, dropout_rate, attention_dropout_rate, num_heads):
        super().__init__()
        self.self_attention_norm = nn.LayerNorm(hidden_size)
        self.self_attention = MultiHeadAttention(hidden_size, attention_dropout_rate, num_heads)
        self.self_attention_dropout = nn.Dropout(dropout_rate)
        self.ffn_norm1 = nn.LayerNorm(hidden_size)
        self.ffn_norm2 = nn.LayerNorm(hidden_size)
        self.ffn = FeedForwardNetwork(hidden_size, ffn_size, dropout_rate)
        self.ffn_dropout = nn.Dropout(dropout_rate)

    fused = True
    act_dtype = torch.float32

    def forward(self, x, attn_bias=None, mask=None, next_layer=None):
        if self.fused and x.is_cuda and mask is None:
            return fused_layer_forward(self, "fq", x, attn_bias, self.ffn_norm1, self.ffn_norm2, next_layer=next_layer)
        y = self.self_attention(x, x, x, attn_bias, mask=mask)
        y = self.self_attention_dropout(y)
        x = x + y.to(x.dtype)          # same-dtype add: the mixed fp32+bf16 elementwise kernel is ~20x slower on ROCm
        y = self.ffn_norm1(x)
        y = self.ffn(y)
        y = self.ffn_dropout(y)
        x = x + y.to(x.dtype)          # same-dtype add: the mixed fp32+bf16 elementwise kernel is ~20x slower on ROCm
        return self.ffn_norm2(x)


def load_universe(dataset_name, root=".."):
    """Read what the reference constructor reads (model_fqandtoyo.py:650-700 / 787-838, 893 / 772): the four
    Graph_*.csv files and the POI distance pickle, relative to `root` (the reference uses cwd = graphormer/)."""
    import pandas as pd
    from .synth import Universe
    path = os.path.join(root, "dataset", dataset_name, "raw")
    raw_X = pd.read_csv(os.path.join(path, "Graph_poi.csv"))
    pkl = {"foursquaregraph": "tky_distance.pkl", "gowalla_nevda": "gowalla_distance.pkl",
           "gowalla_7day": "gowalla_distance.pkl"}[dataset_name]
    with open(os.path.join(root, "dataset", "poi_data", pkl), "rb") as f:
        dist = pickle.load(f, encoding="iso-8859-1")
    return Universe(P=len(raw_X), n_cat=0, n_user=0, poi_table=raw_X.to_numpy().astype(np.float64),
                    graph_adj=pd.read_csv(os.path.join(path, "Graph_adj.csv")).to_numpy(),
                    graph_dist=pd.read_csv(os.path.join(path, "Graph_dist.csv")).to_numpy(),
                    graph_cat=pd.read_csv(os.path.join(path, "Graph_cat.csv")).to_numpy(),
                    distance=np.asarray(dist), poi_columns=tuple(raw_X.columns))


class Graphormer(nn.Module):
    """model_fqandtoyo.py:580-1432 for dataset_name in {foursquaregraph, gowalla_nevda, gowalla_7day}.
    `universe` (a `synth.Universe`) replaces the CSV / pickle reads when given; `num_bins` overrides the
    Freedman-Diaconis bin count (needed when no distance matrix is materialised, e.g. P = 100k)."""

    def __init__(self, n_layers, num_heads, hidden_dim, dropout_rate, intput_dropout_rate, weight_decay, ffn_dim,
                 dataset_name, warmup_updates, tot_updates, peak_lr, end_lr, edge_type, multi_hop_max_dist,
                 attention_dropout_rate, flag=False, flag_m=3, flag_step_size=1e-3, flag_mag=1e-3, lr_step=2,
                 universe=None, num_bins=None, bias_dtype=torch.float32, gcn_dtype=torch.float32,
                 act_dtype=torch.float32, fused_layers=True):
        super().__init__()
        if dataset_name not in ("foursquaregraph", "gowalla_nevda", "gowalla_7day", "toyotagraph"):
            raise NotImplementedError(f"dataset_name={dataset_name!r}: only the POI-graph datasets are in scope")
        if edge_type != "multi_hop":
            raise NotImplementedError("only edge_type='multi_hop' is used by MobGT (README.md:62)")
        fsq = dataset_name == "foursquaregraph"
        # `toyotagraph` (model_fqandtoyo.py:902-1039; README.md:72-83): the gowalla-style body with 995 + 1 user rows, a plain
        # 48-slot time table (no padding row), no cat_embed_model, a num_cats-way category head, a log_softmax POI head
        # (:1417-1428) and loss = GradientTailLoss(category logits, category of the target, 0.1) + NLLLoss(ignore_index=0) (:1462-1471)
        toyota = dataset_name == "toyotagraph"
        self.num_virtual_tokens = 1
        self.num_heads = num_heads
        self.dataset_name = dataset_name
        self.edge_type = edge_type
        self.edge_encoder = nn.Embedding(128, num_heads, padding_idx=0)
        self.edge_dis_encoder = nn.Embedding(128 * num_heads * num_heads, 1)
        self.rel_pos_encoder = nn.Embedding(512, num_heads, padding_idx=0)
        if fsq:
            self.time_encoder = nn.Embedding(48, 512)                 # unused in forward (:786)

        uni = universe if universe is not None else load_universe(dataset_name)
        raw_X = uni.poi_table
        P = raw_X.shape[0]
        cats = raw_X[:, 4]
        uniq = np.unique(cats)                                        # sklearn OneHotEncoder: sorted categories
        num_cats = len(uniq)
        onehot = (cats[:, None] == uniq[None, :]).astype(np.float32)
        X = np.zeros((P, 3 + num_cats), dtype=np.float32)
        X[:, 0] = raw_X[:, 1]
        X[:, 1:num_cats + 1] = onehot
        X[:, num_cats + 1] = raw_X[:, 2]
        X[:, num_cats + 2] = raw_X[:, 3]
        C_X = (np.arange(1, num_cats + 1)[:, None] == uniq[None, :]).astype(np.float32)
        self.register_buffer("X", torch.from_numpy(X), persistent=False)
        self.register_buffer("C_X", torch.from_numpy(C_X), persistent=False)
        graph_dist, radius_graph = uni.graph_dist, None
        from .geo import RadiusGraph
        if isinstance(graph_dist, RadiusGraph):
            # built from coordinates on the device (geo.radius_graph): the adjacency tensors are registered as they lie there;
            # everything computed ONCE from the graph on the host (D_AX, the dense D_A of the bitmask configuration) is computed
            # from its host copy exactly as for a universe read from disk, so every buffer has the bits it has today.  The
            # bitmask configuration needs the bit words and the bf16 GCN; anything else takes the CSR path
            radius_graph = graph_dist
            if gcn_dtype == torch.bfloat16 and "mask" in radius_graph.forms:
                graph_dist = radius_graph.to_dense01()
            else:
                radius_graph.require("csr")
                graph_dist = radius_graph.to_scipy()
        self.sparse_adj = not isinstance(graph_dist, np.ndarray)
        if self.sparse_adj:
            # P too large for a dense P x P adjacency (S-BIG: 100 000 POIs): the same (D+I)^-1 (A+I) as CSR, its transpose
            # as CSR, A.X once on the host (scipy); the GCN then runs on csrc/spmm.hip (modelGNN.CsrAdj)
            from scipy import sparse
            from .modelGNN import CsrAdj
            a = sparse.csr_matrix(graph_dist, dtype=np.float64)
            deg = np.asarray(a.sum(axis=1)).reshape(-1) + 1.0
            a_hat = sparse.diags(1.0 / deg) @ (a + sparse.identity(P, format="csr"))
            self.register_buffer("D_AX", torch.from_numpy(np.asarray(a_hat @ X.astype(np.float64), dtype=np.float32)), persistent=False)
            for name, t in zip(("D_A_rowptr", "D_A_col", "D_A_val", "D_AT_rowptr", "D_AT_col", "D_AT_val"),
                               radius_graph.csr_adj() if radius_graph is not None else CsrAdj.from_scipy(a_hat)):
                self.register_buffer(name, t, persistent=False)
            self.D_A = self.D_A_T = None
            self.D_mask = self.D_mask_t = self.D_scale = None
        else:
            d_a = torch.from_numpy(calculate_laplacian_matrix(graph_dist)).float()
            # A.X for the constant POI feature matrix, once, in fp32 (see modelGNN.GCN.forward)
            d_ax = d_a @ torch.from_numpy(X)
            self.register_buffer("D_A", d_a.to(gcn_dtype), persistent=False)
            # the constant's transpose, stored once: the backward's adj^T @ g then streams rows like the forward
            self.register_buffer("D_A_T", d_a.t().contiguous().to(gcn_dtype) if gcn_dtype != torch.float32 else None,
                                 persistent=False)
            # bf16 configuration: the 0/1 structure of the adjacency as a bitmask + row scale (modelGNN.MaskAdj); the
            # hidden GraphConvolution layers then never stream the dense matrix (the rows-only last layer still gathers
            # its <= G*N rows from it)
            packed = None
            if gcn_dtype == torch.bfloat16:
                from .modelGNN import MaskAdj
                packed = radius_graph.mask_adj() if radius_graph is not None else MaskAdj.from_dense01(graph_dist)
            if packed is not None and d_ax.shape[1] % 16:
                # bitmask configuration: A X zero-padded to whole 16-deep k-steps (303 -> 304 columns) for the first
                # GraphConvolution's GEMM + activation node (modelGNN._ConvActFn); GCN.forward slices it for any other path
                self._d_ax_pad = 16 - d_ax.shape[1] % 16
                d_ax = torch.nn.functional.pad(d_ax, (0, self._d_ax_pad))
            self.register_buffer("D_AX", d_ax.contiguous(), persistent=False)
            for name, t in zip(("D_mask", "D_mask_t", "D_scale"), packed if packed is not None else (None, None, None)):
                self.register_buffer(name, t, persistent=False)
        c_a = torch.from_numpy(calculate_laplacian_matrix(uni.graph_cat)).float()
        self.register_buffer("C_A", c_a, persistent=False)
        self.register_buffer("C_A_T", c_a.t().contiguous(), persistent=False)
        self.register_buffer("C_AX", c_a @ torch.from_numpy(C_X), persistent=False)
        # POI id (1..P) -> category id (1..n_cat); row 0 = pad.  Replaces poi_idx2cat_idx_dict (:1106-1108)
        poi2cat = np.zeros(P + 1, dtype=np.int64)
        poi2cat[raw_X[:, 0].astype(np.int64)] = cats.astype(np.int64)
        self.register_buffer("poi2cat", torch.from_numpy(poi2cat), persistent=False)
        if fsq:
            self.atom_encoder = nn.Embedding(P, hidden_dim, padding_idx=0)   # unused in forward (:811)

        self.gcn_nfeat, self.gcn_nhid = X.shape[1], [16, 64]
        self.poi_embed_model = GCN(ninput=self.gcn_nfeat, nhid=self.gcn_nhid, noutput=hidden_dim, dropout=0.3)  # unused
        self.fuse_embed = nn.Linear(2 * hidden_dim, hidden_dim)                                                  # unused
        self.user_embed_dim = self.poi_embed_dim = hidden_dim
        self.time_embed_dim = self.cat_embed_dim = 32
        self.num_users = 937 if dataset_name == "gowalla_7day" else (996 if toyota else 1080)     # (:1002: UserEmbeddings(995 + 1))
        self.poi_distance_model = GCN(ninput=self.gcn_nfeat, nhid=self.gcn_nhid, noutput=hidden_dim, dropout=0.3)
        if getattr(self, "_d_ax_pad", 0):
            # the first layer's weight gradient is computed with the rows of zero products of the padded A X: room for them behind
            # the gradient's slot in a trainer's flat buffer (train.flat_offsets)
            w0 = self.poi_distance_model.gcn[0].weight
            w0._mobgt_flat_slack = self._d_ax_pad * w0.shape[1]
        self.poi_cat_model = GCN(ninput=C_X.shape[1], nhid=self.gcn_nhid, noutput=self.cat_embed_dim, dropout=0.1)
        self.user_embed_model = UserEmbeddings(self.num_users, self.user_embed_dim)
        self.time_embed_model_48 = nn.Embedding(48 + 1 if fsq else 48, self.time_embed_dim, padding_idx=None if toyota else 0)
        if not toyota:
            self.cat_embed_model = CategoryEmbeddings(num_cats if fsq else num_cats + 1, self.cat_embed_dim)    # unused
        C = hidden_dim + self.time_embed_dim + self.cat_embed_dim
        Cout = hidden_dim * 2 + self.time_embed_dim + self.cat_embed_dim
        self.cat_decoder = nn.Linear(Cout, num_cats if (fsq or toyota) else num_cats + 1)
        self.embed_fuse_model1 = FuseEmbeddings(self.user_embed_dim, self.poi_embed_dim)                         # unused
        self.embed_fuse_model2 = FuseEmbeddings(self.poi_embed_dim, self.time_embed_dim)
        self.embed_fuse_model3 = FuseEmbeddings(self.user_embed_dim, C)
        self.embed_fuse_model4 = FuseEmbeddings(self.poi_embed_dim + self.time_embed_dim, self.cat_embed_dim)
        self.pos_embed = LearnablePositionalEncoding(node_dim, C)
        self.in_degree_encoder = nn.Embedding(128, C, padding_idx=0)
        self.out_degree_encoder = nn.Embedding(128, C, padding_idx=0)
        freq_col = list(uni.poi_columns).index("checkin_cnt" if dataset_name == "gowalla_7day" else "check_freq")
        self.fre_embed_model = nn.Embedding(int(raw_X[:, freq_col].max()) + 1, C, padding_idx=0)
        self.output_dropout = nn.Dropout(intput_dropout_rate)
        if num_bins is None:
            d = uni.distance
            dm = np.delete(d, 0, axis=0)
            if not fsq:
                dm = np.delete(dm, 0, axis=1)        # the foursquaregraph branch discards its column delete (:894)
            num_bins = freedman_diaconis_bins(dm - dm.min())
        self.poi_pos_encoder = nn.Embedding(num_bins, num_heads, padding_idx=0)

        self.input_dropout = nn.Dropout(intput_dropout_rate)
        self.layers = nn.ModuleList([EncoderLayer(C, ffn_dim, dropout_rate, attention_dropout_rate, num_heads)
                                     for _ in range(n_layers)])
        for li, layer in enumerate(self.layers):
            layer.act_dtype, layer.fused = act_dtype, fused_layers
            layer.self_attention.set_layer_index(li + 1)
        self.act_dtype = act_dtype
        for m in (self.embed_fuse_model2, self.embed_fuse_model3, self.embed_fuse_model4):
            m.bf16_wgrad = act_dtype == torch.bfloat16       # bf16 configuration: weight gradients with bf16 MFMA operands
        self.final_ln = nn.LayerNorm(Cout)
        self.out_proj = nn.Linear(Cout, P if fsq else P + 1)
        self.ELU = nn.ELU()
        self.graph_token = nn.Embedding(self.num_virtual_tokens, C)
        self.graph_token_virtual_distance = nn.Embedding(self.num_virtual_tokens, num_heads)

        self.warmup_updates, self.tot_updates = warmup_updates, tot_updates
        self.peak_lr, self.end_lr, self.weight_decay = peak_lr, end_lr, weight_decay
        self.multi_hop_max_dist = multi_hop_max_dist
        self.hidden_dim = hidden_dim
        self.bias_dtype = bias_dtype
        self.gcn_dtype = gcn_dtype
        # NB: the reference's `self.apply(init_bert_params)` is commented out here (:1099): default torch init.

    # ------------------------------------------------------------------------------------------------
    def _hop_depth(self, batched_data):
        D = batched_data.edge_input.shape[3]
        return min(D, self.multi_hop_max_dist) if self.multi_hop_max_dist > 0 else D

    def hop_table(self, batched_data):
        """The [D, n_edge, H] table of edge feature x hop distance products (:1178-1198, once per batch instead of per pair)."""
        return hop_table_from(self.edge_encoder.weight, self.edge_dis_encoder.weight, self.num_heads, self._hop_depth(batched_data),
                              fp16_roundtrip=True)

    def gather_indices(self, batched_data):
        """Every gather index of :1259-1264 / :1287-1298 in one launch: POI row (in the compact per-batch table when rows_only:
        row p belongs to position p), time slot (:1262), category row (:1259), positional row 1..n (:348-351), GCN row, zeros."""
        x = batched_data.x[:, :, 0]                                           # [G,N] POI ids, 0 = pad
        if x.dtype not in (torch.int64, torch.int32):
            x = x.long()
        G, N = x.shape
        # the table is read at <= G*N rows (:1264): compute only those.  The row gather of the dense adjacency pays below P/2
        # rows; the bitmask-rows form of round 4 (modelGNN._DistGcnFn: 1 KB per row, K-split) up to P rows
        mask_rows = (getattr(self, "D_mask", None) is not None and not self.sparse_adj
                     and forms.on("dist_gcn_fused"))
        rows_only = G * N * 2 <= self.X.shape[0] or (mask_rows and G * N <= min(self.X.shape[0], 4096))
        idx, real = ops.node_index(x, batched_data.time_normal[:, :, 0].float(), self.poi2cat, rows_only,
                                   batched_data.in_degree, batched_data.out_degree)
        return idx, real, rows_only

    def assemble_bias(self, batched_data, hop=None):
        """model_fqandtoyo.py:1143-1216 -> ops.PackedBias (fp16 rounding points of :1178-1198 kept)."""
        edge_input = batched_data.edge_input
        D = self._hop_depth(batched_data)
        if hop is None:
            hop = self.hop_table(batched_data)
        return ops.build_bias(batched_data.attn_bias, batched_data.rel_pos, batched_data.poi_pos, edge_input,
                              # (padding_idx = 0: build_bias_bwd never adds into row 0 of these two tables, so the
                              # tables go in as they are -- no cat / split / zero-fill launches around the kernel)
                              self.rel_pos_encoder.weight, self.poi_pos_encoder.weight, hop,
                              self.graph_token_virtual_distance.weight, D, dtype=self.bias_dtype)

    def node_features(self, batched_data, indices=None):
        """model_fqandtoyo.py:1222-1342 -> [G, N+1, C] (graph token first)."""
        G, N = batched_data.x.shape[:2]
        idx, real, rows_only = indices if indices is not None else self.gather_indices(batched_data)
        poi_idx, time_idx, cat_idx, pos_idx, gcn_rows, zero_idx, in_deg, out_deg = idx.unbind(0)
        if self.sparse_adj:
            from .modelGNN import CsrAdj
            adj = CsrAdj(self.D_A_rowptr, self.D_A_col, self.D_A_val, self.D_AT_rowptr, self.D_AT_col, self.D_AT_val)
            poidist = self.poi_distance_model(self.X, adj, self.D_AX, rows=gcn_rows.reshape(-1) if rows_only else None)
        else:
            mask_adj = None
            if getattr(self, "D_mask", None) is not None:
                from .modelGNN import MaskAdj
                mask_adj = MaskAdj(self.D_mask, self.D_mask_t, self.D_scale)
            poidist = self.poi_distance_model(self.X, self.D_A, self.D_AX, rows=gcn_rows.reshape(-1) if rows_only else None,
                                              adj_t=self.D_A_T, mask_adj=mask_adj, parts_ok=G * N <= 4096)   # :1236
        ops.trace_nan("poidist", poidist)
        catemb = self.poi_cat_model(self.C_X, self.C_A, self.C_AX, adj_t=self.C_A_T)                                    # :1237
        Wp, Wt, Wc, C = poidist.shape[1], self.time_embed_model_48.weight.shape[1], catemb.shape[1], self.pos_embed.pe.shape[1]
        f4 = self.embed_fuse_model4
        one_launch = G * N <= 4096
        # the first encoder layer's QKV projection rides in the token-assembly launch when its packed weights are current (chain
        # kernels) -- and then (round 4) so do the gathers and the two FuseEmbeddings layers below: they only record their
        # launches (ops.token_fwd_deferral), ops.assemble_tokens issues mobgt_token_fwd_chain for all of them
        l0 = self.layers[0]
        first_qkv = None
        if (getattr(l0, "fused", False) and getattr(l0, "_packed_fresh", False) and getattr(l0, "act_dtype", None) == torch.bfloat16
                and not torch.is_autocast_enabled("cuda")):
            first_qkv = (l0._packed[0], l0._shadows[1])
        ops.token_fwd_deferral(one_launch and first_qkv is not None and self.act_dtype == torch.bfloat16 and C == 192 and Wp + Wt == 160)
        try:
            return self._node_features_tail(batched_data, G, N, poidist, catemb, real, one_launch, first_qkv, Wp, Wt, Wc, C,
                                            poi_idx, time_idx, cat_idx, pos_idx, zero_idx, in_deg, out_deg, rows_only)
        finally:
            ops.token_fwd_deferral(False)

    def _node_features_tail(self, batched_data, G, N, poidist, catemb, real, one_launch, first_qkv, Wp, Wt, Wc, C,
                            poi_idx, time_idx, cat_idx, pos_idx, zero_idx, in_deg, out_deg, rows_only=False):
        f4 = self.embed_fuse_model4
        if one_launch:
            # every gathered row of :1259-1298 in ONE launch: [poi ; time] -> pt, the category row -> the trailing columns of
            # fuse4's input, fre_embed(0) + degree rows + positional rows pe[1..n] (:1287-1298, :348-351) summed -> add
            pt, x4, add = ops.embed_gather_multi(
                [(poidist, poi_idx, 0, 0, False, None)] +
                # (round 4: the distance GCN's output may arrive as partial tables -- modelGNN._DistGcnFn -- added here, in order)
                [(part, poi_idx, 0, 0, 2, None) for part in getattr(poidist, "_mobgt_parts", ())] +
                [(self.time_embed_model_48.weight, time_idx, 0, Wp, False, self.time_embed_model_48.padding_idx),
                 (catemb, cat_idx, 1, Wp + Wt, False, None),
                 (self.fre_embed_model.weight, zero_idx, 2, 0, False, 0), (self.in_degree_encoder.weight, in_deg, 2, 0, True, 0),
                 (self.out_degree_encoder.weight, out_deg, 2, 0, True, 0), (self.pos_embed.pe, pos_idx, 2, 0, True, None)],
                [Wp + Wt, Wp + Wt + Wc, C],
                # (the fused distance GCN's compact per-batch table: row p belongs to position p -- gather_indices, ops.node_index)
                identity=0 if (rows_only and hasattr(poidist, "_mobgt_parts") and poidist.shape[0] == G * N) else None)
            # fuse2 (:1268) writes straight into the leading columns of fuse4's input (:1269): no torch.cat
            f2 = ops.linear_splitk(pt, self.embed_fuse_model2.fuse_embed.weight, self.embed_fuse_model2.fuse_embed.bias,
                                   self.act_dtype == torch.bfloat16, slope=self.embed_fuse_model2.leaky_relu.negative_slope,
                                   out=x4[:, :Wp + Wt])
            if f2.data_ptr() == x4.data_ptr():
                x4 = ops.join_cols(x4, f2)
            else:                                                               # (the library path wrote elsewhere)
                x4 = torch.cat((f2, x4[:, Wp + Wt:]), 1)
            nf = ops.linear_splitk(x4, f4.fuse_embed.weight, f4.fuse_embed.bias, getattr(f4, "bf16_wgrad", False),
                                   slope=f4.leaky_relu.negative_slope)
            if f2.data_ptr() == x4.data_ptr() and self.act_dtype == torch.bfloat16 and getattr(f4, "bf16_wgrad", False):
                # the backward of tokens <- nf <- x4 <- pt as ONE launch inside the trainer's step (csrc/tokbwd.hip)
                ops.register_token_chain(nf, x4, Wp + Wt, f4.fuse_embed.weight, f4.leaky_relu.negative_slope,
                                         self.embed_fuse_model2.fuse_embed.weight, self.embed_fuse_model2.leaky_relu.negative_slope)
        else:
            # many positions (S-BIG: 12.5 k rows): the separate gathers, whose backward combines runs of equal indices in
            # registers (scatter_add_runs_kernel) instead of serialising thousands of atomics on a handful of degree rows
            pt = ops.embed_gather_concat([poidist, self.time_embed_model_48.weight], [poi_idx, time_idx],
                                         padding_idx=[None, self.time_embed_model_48.padding_idx])
            f2 = ops.linear_splitk(pt, self.embed_fuse_model2.fuse_embed.weight, self.embed_fuse_model2.fuse_embed.bias,
                                   self.act_dtype == torch.bfloat16, slope=self.embed_fuse_model2.leaky_relu.negative_slope)
            nf = f4(f2, ops.embed_gather_sum([catemb], [cat_idx]))
            add = ops.embed_gather_sum(
                [self.fre_embed_model.weight, self.in_degree_encoder.weight, self.out_degree_encoder.weight, self.pos_embed.pe],
                [zero_idx, in_deg, out_deg, pos_idx], padding_idx=[0, 0, 0, None])
        ops.trace_nan("pt", pt)
        ops.trace_nan("f2", f2)
        ops.trace_nan("fuse4", nf)
        # (pads stay 0: the multiplication by `real` happens inside assemble_tokens)
        # nf * real + add -> pos_embed dropout (:358); graph token + pe[0] -> the same dropout (:1338-1342); cat;
        # input_dropout (:1347): one launch
        return ops.assemble_tokens(nf.view(G, N, -1), real, add.view(G, N, -1), self.graph_token.weight, self.pos_embed.pe, self.pos_embed.dropout.p,
                                   self.input_dropout.p, self.training,
                                   bf16_copy=self.act_dtype == torch.bfloat16 and getattr(self.layers[0], "fused", False),
                                   pe_row0_via_gather=one_launch, first_qkv=first_qkv)

    def validate_batch(self, batched_data):
        """Index ranges nn.Embedding would check in the reference (IndexError there; the gather kernels here do not
        bounds-check per element).  One reduction + one host read per batch OBJECT, remembered on it -- so a
        pre-collated batch is checked in the eager dry run and costs nothing inside a captured step."""
        if getattr(batched_data, "_mobgt_validated", None) is self or not batched_data.x.is_cuda:
            return
        if torch.cuda.is_current_stream_capturing():
            return
        P = self.X.shape[0]
        lim = [("x", batched_data.x, P + 1), ("in_degree", batched_data.in_degree, self.in_degree_encoder.num_embeddings),
               ("out_degree", batched_data.out_degree, self.out_degree_encoder.num_embeddings),
               ("rel_pos", batched_data.rel_pos, self.rel_pos_encoder.num_embeddings),
               ("poi_pos", batched_data.poi_pos, self.poi_pos_encoder.num_embeddings),
               ("edge_input", batched_data.edge_input, self.edge_encoder.num_embeddings),
               ("user", batched_data.user, self.num_users + 1),
               ("y", batched_data.y, self.out_proj.out_features + 1)]
        mx = torch.stack([t.max().long() if t.numel() else torch.zeros((), dtype=torch.long, device=t.device)
                          for _, t, _ in lim]).tolist()
        tmax = float(batched_data.time_normal.max()) if batched_data.time_normal.numel() else 0.0
        for (name, _, n), m in zip(lim, mx):
            if m >= n:
                raise IndexError(f"batch.{name} has index {m}, out of range for a table of {n} rows")
        if int(tmax * 48) >= self.time_embed_model_48.num_embeddings:
            raise IndexError(f"batch.time_normal {tmax} maps to a time slot outside the {self.time_embed_model_48.num_embeddings}-row table")
        try:
            batched_data._mobgt_validated = self
        except AttributeError:
            pass

    def index_limits(self):
        """Largest admissible value + 1 of the raw fields train.EpochLoop checks on the host for a fresh batch."""
        return dict(x=self.X.shape[0], user=self.num_users, y=self.out_proj.out_features, edge=self.edge_encoder.num_embeddings,
                    deg=self.in_degree_encoder.num_embeddings, slots=self.time_embed_model_48.num_embeddings)

    def encode(self, batched_data):
        """The batch -> tok [G, C + U], the classifier heads' input (:1143-1364): everything but the two output Linears.  Leaves
        `_bias_pack`, `_cuts` and `_enc_out` on the module for train.TrainStep, which cuts the backward pass there."""
        self.validate_batch(batched_data)
        # The category GCN (weights only: no batch input; one launch that keeps 19 compute units busy) goes FIRST and carries the
        # step's other front-of-step launches as passenger workgroups: the hop table's forward, the gather indices, the MFMA-order
        # pack of the layer weights.  Their ops only leave jobs here (front_deferral / defer_pack); the flushes below launch alone
        # whatever the GCN could not take along (no one-launch form for this shape, MOBGT_NO_*_PASSENGER switches).
        ops.front_deferral(True)
        try:
            hop = self.hop_table(batched_data)
            indices = self.gather_indices(batched_data)
        finally:
            ops.front_deferral(False)
        refresh_shadows(self.layers, defer_pack=True, rows=batched_data.x.shape[0] * (batched_data.x.shape[1] + 1))
        prelaunch_small_gcn(self.poi_cat_model, self.C_X, self.C_A, self.C_AX, self.C_A_T, same_stream=True)
        flush_pending_pack()
        ops.flush_front()
        try:
            # (round 4) the distance GCN's first layer, leaky((A X) W0 + b0) over all P POIs -- parameters only, no batch input -- rides
            # in the bias assembly's launch; modelGNN finds its result when it asks ops.small_gemm for this very product
            g0 = self.poi_distance_model.gcn[0]
            if (getattr(self, "D_mask", None) is not None and not self.sparse_adj and self.D_AX.is_cuda and self.D_AX.shape[1] % 16 == 0
                    and g0.out_features == 16 and g0.bias is not None and 0 <= self.D_AX.shape[1] - g0.in_features < 16):
                from .modelGNN import xt_workspace
                ops.front_small_gemm(self.D_AX, g0.weight, g0.bias, float(self.poi_distance_model.leaky_relu.negative_slope),
                                     g0.weight.shape[0], xt_workspace(self.D_AX.device, self.D_AX.shape[0], g0.out_features, slot=0))
            bias = self.assemble_bias(batched_data, hop=hop)
            ops.front_small_gemm_flush()
            output = self.node_features(batched_data, indices=indices)
        except BaseException:
            ops.drop_parked()
            raise
        # (a prelaunched result nobody adopted must not meet a later, direct call of the GCN; the same for a small GEMM's result)
        STEP.gcn_prelaunched.pop(id(self.poi_cat_model), None)
        STEP.front_sgemm.pop("done", None)
        ops.trace_nan("x0", output)
        self._bias_pack, self._cuts = bias, {}
        for li, enc_layer in enumerate(self.layers):                                           # :1347-1352
            if getattr(enc_layer, "_mobgt_cut", False):
                self._cuts[li] = output          # train.TrainStep: the backward pass is cut here (layer-wise gradient buckets)
            # (the layer that follows is named so that its QKV projection can ride in this layer's last launch)
            output = enc_layer(output, bias, mask=None, next_layer=self.layers[li + 1] if li + 1 < len(self.layers) else None)
            ops.trace_nan(f"layer{li}", output)
        self._enc_out = output           # train.TrainStep: everything after this point is the "head" (see head_modules)
        fuse3 = self.embed_fuse_model3
        user = batched_data.user
        if output.is_cuda and self.final_ln.weight.shape[0] <= 512 and output.dtype == torch.float32 \
                and user.dtype in (torch.int64, torch.int32) and user.numel() == output.shape[0]:
            # [graph-token row | user_embed_model(user - 1)] in one launch (:1239-1240), the Linear of FuseEmbeddings,
            # then LeakyReLU -> final_ln -> ELU -> output dropout in ONE launch (:1353-1364)
            utab = self.user_embed_model.user_embedding.weight
            if ops.head_chain_ok(output, utab, user, fuse3.fuse_embed.weight):
                # ... and all three in ONE launch each way (csrc/head.hip)
                tok = ops.head_chain(output, utab, user, -1, fuse3.fuse_embed.weight, fuse3.fuse_embed.bias, self.final_ln.weight,
                                     self.final_ln.bias, self.final_ln.eps, 0.2, self.output_dropout.p, self.training, 0x1004,
                                     bf16_wgrad=getattr(fuse3, "bf16_wgrad", False))
            else:
                x3 = ops.head_input(output, utab, user, -1)
                u3 = ops.linear_splitk(x3, fuse3.fuse_embed.weight, fuse3.fuse_embed.bias, getattr(fuse3, "bf16_wgrad", False))
                tok = ops.head_act(u3, self.final_ln.weight, self.final_ln.bias, self.final_ln.eps, 0.2, self.output_dropout.p,
                                   self.training, 0x1004)
        else:
            user_embedding = self.user_embed_model(user.long() - 1).reshape(output.shape[0], -1)   # :1239-1240
            tok = fuse3(output[:, 0, :].float(), user_embedding)                               # :1353-1358, q = 0 only
            tok = ops.dropout(self.ELU(self.final_ln(tok)), self.output_dropout.p, self.training, 0x1004)   # :1360-1364
        ops.trace_nan("tok", tok)
        return tok

    @property
    def label_offset(self):
        """y - label_offset is y's column of the POI head: 1 for foursquaregraph / gowalla, whose steps rank against y - 1
        (:1446-1460, :1483-1495), 0 for toyotagraph, whose steps take y as it is (:1462-1471).  x holds POI ids as y does."""
        return 0 if self.dataset_name == "toyotagraph" else 1

    def poi_logits(self, tok):
        """:1394 with M = G rows: the skinny classifier where the shape allows it, else out_proj"""
        if ops.skinny_linear_ok(tok, self.out_proj.weight):
            logits = ops.skinny_linear(tok, self.out_proj.weight, self.out_proj.bias)
        else:
            logits = self.out_proj(tok)
        return ops.trace_nan("logits", logits)

    def poi_scores(self, tok):
        """What the reference's steps rank: the POI logits; for toyotagraph the head's log-probabilities (:1417-1428).
        (The logits are stored and ranked by mobgt_rank_metrics: measured faster than the fused classifier-ranking form,
        ops.skinny_linear_rank_metrics, at every width from 3 680 to 100 001 classes -- 15.1 against 23.4 us at S-FSQ's 7 857,
        49 against 75 us at S-BIG's 100 001 (tools/eval_bench.py); both give the same bits.)"""
        logits = self.poi_logits(tok)
        return torch.log_softmax(logits.float(), dim=1) if self.label_offset == 0 else logits

    def forward(self, batched_data, perturb=None):
        tok = self.encode(batched_data)
        return [self.poi_scores(tok), self.cat_decoder(tok)]                                              # :1394-1396 / :1417-1428

    # modules whose parameters only receive gradient from the part of the graph ABOVE the encoder output: their
    # gradients are complete after the first ~20 kernels of the backward pass (61 % of all gradient bytes: out_proj)
    head_modules = ("out_proj", "final_ln", "embed_fuse_model3", "user_embed_model", "cat_decoder")

    def training_step(self, batched_data, batch_idx=0):
        """model_fqandtoyo.py:1446-1460: y-1 targets, GradientTailLoss(alpha=0.2) on the POI logits only (the category decoder,
        whose output the loss does not read, is not run).
        toyotagraph (:1462-1471): GradientTailLoss(category logits, category of the target POI - 1, alpha = 0.1) +
        NLLLoss(ignore_index=0)(log_softmax(POI logits), y) -- y unshifted, the category target as :1262 derives it."""
        tok = self.encode(batched_data)
        if self.dataset_name == "toyotagraph":
            logits, cat_logits = self.poi_logits(tok), self.cat_decoder(tok)
            y = batched_data.y.long().view(-1)
            cat_target = self.poi2cat[y] - 1                                                   # :1262 (poi_idx2cat_idx_dict[y] - 1)
            loss_cat = ops.gradient_tail_loss(cat_logits, cat_target, 0.1, target_offset=0)
            if ops.cross_entropy_ok(logits, y):
                # (mobgt_cross_entropy is NLLLoss(log_softmax(logits)) in one kernel: the log-probabilities are never stored)
                loss_poi = ops.cross_entropy(logits, y, ignore_index=0)
            else:
                loss_poi = F.nll_loss(torch.log_softmax(logits.float(), dim=1), y, ignore_index=0)
            return loss_cat + loss_poi
        if ops.skinny_linear_gtl_ok(tok, self.out_proj.weight):
            # the classifier and the loss in ONE launch; the logits are never stored
            return ops.skinny_linear_gtl(tok, self.out_proj.weight, self.out_proj.bias, batched_data.y, 0.2, target_offset=-1)
        return ops.gradient_tail_loss(self.poi_logits(tok), batched_data.y, 0.2, target_offset=-1)

    def validation_step(self, batched_data, batch_idx=0):
        """model_fqandtoyo.py:1483-1495"""
        return {"y_pred": self(batched_data), "y_true": batched_data.y.long() - 1}

    def test_step(self, batched_data, batch_idx=0):
        """model_fqandtoyo.py:1530-1544"""
        return {"y_pred": self(batched_data), "y_true": batched_data.y.long() - 1, "idx": batched_data.idx}

    def metric_step(self, batched_data, acc, work=None, exclude_visited=False, allow=None, split_revisits=False, near=None,
                    restriction=None, prior=None):
        """validation_step / test_step + test_epoch_end's per-batch bookkeeping in one pass: the batch's ACC / NDCG @1/5/10/20
        and MRR sums (metrics.evaluate_outputs, quirks included) are ADDED to `acc` (metrics.new_accumulator) on the device --
        no category head, no host read.  Eval mode, under no_grad.  toyotagraph ranks log_softmax(logits) against
        the UNSHIFTED y, as the reference's validation / test step does (:1484-1495).  `work`: ops.rank_metrics' buffer.

        Restricted and split (ops.rank_metrics_masked; acc = metrics.new_restricted_accumulator(device, split_revisits), work of
        ops.rank_metrics_masked_work_bytes): the ranking of the lists recommend_step returns with the same exclude_visited /
        allow, so a hit at k <=> y is in that list's first k; a row whose y cannot be listed counts in n only.  split_revisits
        adds the rows whose y is not among the trajectory's POIs (batched_data.x) to slot 1, the others to slot 2.
        near: recommend_step's radius restriction (see there); a y outside its row's radius counts in n only.
        restriction: a prebuilt restriction.Restriction in place of those four keywords (the loops build theirs once).
        prior: any prior (a prior.Prior) or a prior.Stack of them (one launch per member, in its order); a
        MarkovPrior's weighted log-counts are added to the scores, in place, before they are ranked (one launch,
        mobgt_prior_blend_rows; the rule is prior.py's docstring): every restriction then acts on the blended scores."""
        if self.training:
            raise RuntimeError("metric_step: the model is in training mode (call .eval() first)")
        r = restriction or Restriction(self.label_offset, exclude_visited, allow, split_revisits, near)
        with torch.no_grad():
            scores = self.poi_scores(self.encode(batched_data))
            if prior is not None:
                scores = prior.blend(scores, batched_data, self.label_offset)
            if r.active:
                hist = r.hist(batched_data)
                ops.rank_metrics_masked(scores, batched_data.y, acc, target_offset=-r.label_offset, allow=r.allow_for(hist),
                                        hist=hist, hist_offset=r.label_offset, exclude_hist=r.exclude_visited,
                                        split=r.split_revisits, work=work)
            else:
                ops.rank_metrics(scores, batched_data.y, acc, target_offset=-r.label_offset, work=work)
        return acc

    def recommend_step(self, batched_data, ids, vals, work=None, exclude_visited=False, allow=None, near=None, restriction=None,
                       prior=None):
        """The batch's top-k next POIs, best first, into ids [G, k] int64 / vals [G, k] f32 (k = ids.shape[1] <= ops.TOPK_MAX) on
        the device: the scores metric_step ranks (logits; log_softmax for toyotagraph) in ops.topk_rows' order, so equal scores
        list the lower POI first and `y in ids[:, :k]` is exactly the hit ACC@k counts.  ids are in batched_data.y's label space:
        column + 1 for foursquaregraph / gowalla (whose test_step ranks against y - 1), the column itself for toyotagraph.  Eval
        mode, under no_grad; nothing else is stored.  `work`: ops.topk_rows' buffer.

        exclude_visited: leave out the POIs of each trajectory (batched_data.x, the same label space as y) -- next *new* POI
        lists.  allow: ops.pack_allow(candidate ids, V, offset) words (offset 0 for toyotagraph, else 1): only those POIs are
        listed.  A row with fewer than k candidates ends in ids -1 / vals -inf.

        near = (pos, chord2_max, mode, words): only POIs within a radius of the row's anchor are listed.  pos =
        ops.pack_positions(coords, V, offset), chord2_max = ops.chord2_of_km(r), mode "last" / "any", words an int32
        [>= G, >= ceil(V / 32)] device buffer: the step launches ops.near_words on batched_data.x into it (inside a captured
        graph when the step is captured; a shared `allow` is ANDed in) and ranks with the rows' own words.  "last" is the
        trajectory's last node (node_name[-1]): for graphs made from sessions (data.SessionCollator, sessions_to_trajectories,
        gen_pickles.py) nodes are ordered by their last visit, so it is the last history check-in; a hand-made dict stores
        distinct POIs in the order given, where it need not be.  "any" -- within r of anywhere the user has been -- does not
        depend on order.

        restriction: a prebuilt restriction.Restriction in place of those three keywords (the loops build theirs once).
        prior: any prior (a prior.Prior) or a prior.Stack blended into the scores, in place, before the lists are taken (as in metric_step); vals are the
        blended scores."""
        if self.training:
            raise RuntimeError("recommend_step: the model is in training mode (call .eval() first)")
        r = restriction or Restriction(self.label_offset, exclude_visited, allow, near=near)
        with torch.no_grad():
            scores = self.poi_scores(self.encode(batched_data))
            if prior is not None:
                scores = prior.blend(scores, batched_data, self.label_offset)
            hist = r.hist(batched_data)
            ops.topk_rows(scores, ids.shape[1], col_offset=r.label_offset, work=work, out=(ids, vals), allow=r.allow_for(hist),
                          exclude=r.exclude(hist))
        return ids, vals

    def recommend(self, dataset, collator, k=20, exclude_visited=False, candidates=None, within_km=None, coords=None, near="last",
                  prior=None, **kw):
        """train.PredictLoop(self, collator, dataset, k=k, exclude_visited=..., candidates=..., within_km=..., coords=...,
        near=..., **kw).run(): (sample_index [n], ids [n, k], vals [n, k]) on the device.  within_km: only POIs within that many
        km of the trajectory's last node (near="last": the last history check-in for sessions and graphs made from them, see
        recommend_step) or of any of its POIs (near="any"); coords [P + 1, 2] lat / lon in degrees, default the collator's.
        prior: a prior.MarkovPrior (mb.prior(...)), a geoprior.DistancePrior (mb.distance_prior(pair_bins)) or a prior.Stack of
        both, blended into the scores before the lists are taken.
        dataset / collator: trajectory dicts with a DeviceCollator, or a data.SessionDataset with a data.SessionCollator."""
        from .train import PredictLoop
        max_batches = kw.pop("max_batches", None)
        return PredictLoop(self, collator, dataset, k=k, exclude_visited=exclude_visited, candidates=candidates,
                           within_km=within_km, coords=coords, near=near, prior=prior, **kw).run(max_batches=max_batches)

    def evaluate(self, dataset, collator, exclude_visited=False, candidates=None, split_revisits=False, within_km=None, coords=None,
                 near="last", prior=None, **kw):
        """train.EvalLoop(self, collator, dataset, exclude_visited=..., candidates=..., split_revisits=..., within_km=...,
        coords=..., near=..., **kw).run(): the reference's validation / test protocol over a whole split, optionally over
        restricted lists (within_km / coords / near as in recommend) and split by revisits.  prior: any prior (a
        prior.Prior) or a prior.Stack blended into the scores before they are ranked.  dataset / collator as in recommend."""
        from .train import EvalLoop
        max_batches = kw.pop("max_batches", None)
        return EvalLoop(self, collator, dataset, exclude_visited=exclude_visited, candidates=candidates,
                        split_revisits=split_revisits, within_km=within_km, coords=coords, near=near, prior=prior,
                        **kw).run(max_batches=max_batches)

    def test_epoch_end(self, outputs):
        """model_fqandtoyo.py:1546-1597: ACC / NDCG @1/5/10/20 and MRR over all test samples."""
        from .metrics import evaluate_outputs
        return evaluate_outputs(outputs)

    def configure_optimizers(self, capturable=False, fused=None):
        """model_fqandtoyo.py:1599-1616"""
        kw = {}
        if capturable:
            kw["capturable"] = True
        if fused is not None:
            kw["fused"] = fused
        optimizer = torch.optim.AdamW(self.parameters(), lr=self.peak_lr, weight_decay=self.weight_decay, **kw)
        scheduler = PolynomialDecayLR(optimizer, warmup_updates=self.warmup_updates, tot_updates=self.tot_updates,
                                      lr=self.peak_lr, end_lr=self.end_lr, power=1.0)
        return [optimizer], [{"scheduler": scheduler, "name": "learning_rate", "interval": "step", "frequency": 1}]
