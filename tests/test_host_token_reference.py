"""tests/token_reference.py without a GPU: the stage-wise float64 reference, composed end to end, IS the model's expressions under
torch autograd (F.embedding, F.linear, F.leaky_relu, a multiplication by mask / keep) on every case of the GPU matrix, for the
values and all gradients; the verdicts of tests/test_gpu_token_matrix.py accept a correct result and reject every deliberately wrong
one of token_reference.MUTANTS on the smallest cases; and every case holds what it claims to exercise (dropped and kept elements at
every dropout site, negative activations, padded nodes, negative indices, padding rows), so none can pass vacuously."""
import pytest
import torch
import torch.nn.functional as F

import token_reference as tr

F64 = torch.float64
FUSED_SPECS = tr.fwd_specs() + tr.bwd_specs()
ALL_SPECS = FUSED_SPECS + tr.assemble_specs() + tr.gather_specs()


def rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30) if b.numel() else 0.0


def autograd(c):
    """The same expressions through torch: -> values and gradients of sum(out * dout)."""
    leaf = lambda t: t.clone().requires_grad_(True)                                           # noqa: E731
    live = [j for j in c.jobs if j.accum != 2]
    tabs = [leaf(j.table) for j in live]
    w2, b2, w4, b4, token = leaf(c.w2), leaf(c.b2), leaf(c.w4), leaf(c.b4), leaf(c.token)
    width = {0: c.W2, 1: c.C, 2: c.C}
    bufs = {s: torch.zeros(c.R, w, dtype=F64) for s, w in width.items()}
    k = -1
    for j in c.jobs:
        if j.accum != 2:
            k += 1
        table = tabs[k] if j.accum != 2 else j.table                                          # (a folded table: a constant)
        e = F.embedding(j.idx.clamp(min=0), table, padding_idx=j.skip if (j.skip >= 0 and j.accum != 2) else None)
        e = e * (j.idx >= 0).to(F64)[:, None]
        bufs[j.slot] = bufs[j.slot] + F.pad(e, (j.coff, width[j.slot] - j.coff - j.width))
    pt, add = bufs[0], bufs[2]
    f2 = F.leaky_relu(F.linear(pt, w2, b2), c.slope2)
    x4 = torch.cat((f2, bufs[1][:, c.W2:]), 1)
    nf = F.leaky_relu(F.linear(x4, w4, b4), c.slope4)
    pe0 = tabs[tr.live_index(c, c.pos_job)][0]
    tok = ((token + pe0).expand(c.G, 1, c.C) * c.keep_tok.reshape(c.G, 1, c.C)) * c.ik_pos
    node = ((nf.reshape(c.G, c.N, c.C) * c.real.reshape(c.G, c.N, 1) + add.reshape(c.G, c.N, c.C)) * c.keep_nf.reshape(c.G, c.N, c.C)) * c.ik_pos
    out = torch.cat((tok, node), 1) * c.keep_in.reshape(c.G, c.T, c.C) * c.ik_in
    for t in (pt, x4, nf, add):
        t.retain_grad()
    (out * c.dout).sum().backward()
    z = lambda t, like: t.grad if t.grad is not None else torch.zeros_like(like)              # noqa: E731
    return dict(pt=pt.detach(), f2=f2.detach(), x4=x4.detach(), nf=nf.detach(), add=add.detach(), out=out.detach(),
                d_pt=z(pt, pt), dx4=z(x4, x4), d_add=z(add, add), d_token=z(token, token),
                dw2=z(w2, w2), db2=z(b2, b2), dw4=z(w4, w4), db4=z(b4, b4), d_tables=[z(t, t) for t in tabs])


@pytest.mark.parametrize("spec", FUSED_SPECS, ids=tr.spec_id)
def test_stagewise_reference_is_autograd(spec):
    c = tr.cached_case(spec)
    f = tr.forward(c)
    b = tr.backward(c, f)
    a = autograd(c)
    for n in ("pt", "f2", "x4", "nf", "add", "out"):
        assert rel(getattr(f, n), a[n]) <= 1e-12, (n, rel(getattr(f, n), a[n]))
    for n in ("d_pt", "dx4", "d_add", "d_token", "dw2", "db2", "dw4", "db4"):
        assert rel(getattr(b, n), a[n]) <= 1e-12, (n, rel(getattr(b, n), a[n]))
    assert len(b.d_tables) == len(a["d_tables"])
    for k, (x, y) in enumerate(zip(b.d_tables, a["d_tables"])):
        assert rel(x, y) <= 1e-12, ("d_table", k, rel(x, y))
    # d_nf is the gradient of nf itself wherever the node is real, and zero on padding
    g4 = b.d_nf * tr.leaky_grad(f.nf, c.slope4)
    assert rel(g4 @ c.w4, a["dx4"]) <= 1e-12
    assert float((b.d_nf[c.real == 0]).abs().sum()) == 0.0
    # the bf16 rows' projection
    rows = f.out.to(torch.bfloat16).to(F64)
    assert rel(tr.qkv_of(c, rows), F.linear(rows.reshape(-1, c.C), c.wq, c.bq)) <= 1e-12


def test_leaky_grad_at_zero_is_the_slope():
    x = torch.tensor([-1.0, 0.0, 2.0], dtype=F64, requires_grad=True)
    F.leaky_relu(x, 0.1).sum().backward()
    assert torch.equal(x.grad, tr.leaky_grad(F.leaky_relu(x.detach(), 0.1), 0.1))
    assert float(x.grad[1]) == 0.1


@pytest.mark.parametrize("spec", ALL_SPECS, ids=tr.spec_id)
def test_cases_hold_what_they_claim(spec):
    c = tr.cached_case(spec)
    both = lambda m: bool(m.any()) and not bool(m.all())                                      # noqa: E731
    if c.p_pos:
        assert both(c.keep_tok == 0) and (c.R == 0 or both(c.keep_nf == 0))
    if c.p_in:
        assert both(c.keep_in == 0)
    if c.p_pos and c.p_in and c.R:
        s = tr.scale_f32(c)
        assert bool((s == 0).any()) and bool((s > 1.2).any())                                 # dropped, and kept by both sites
    if spec["pad"] != "full" and c.N > 0:
        assert "padded" in c.claims
    if "padded" in c.claims:
        assert bool((c.real == 0).any())
    if spec["pad"] == "mixed" and c.G >= 3:
        assert sorted(set(c.lengths)) == sorted({0, 1, c.N})
    if c.C != tr.C_FUSED or c.R == 0:
        return
    f = tr.forward(c)
    assert bool((f.f2 < 0).any()) and bool((f.nf < 0).any())
    live = [j for j in c.jobs if j.accum != 2]
    for j in live:
        assert bool((j.idx[c.real == 0] == -1).all()), "padding: every index -1"
        assert int(j.idx.max()) < j.table.shape[0]
        if c.R >= 4:
            assert bool((j.idx < 0).any()), (j.name, "no negative index")
        if "negatives" in c.claims and int((c.real > 0).sum()) >= 2:
            assert bool((j.idx[c.real > 0] < 0).any()), (j.name, "no negative index on a real node")
            if j.skip >= 0:
                assert bool((j.idx == j.skip).any()), (j.name, "no padding row")
    if "padded" in c.claims:
        pad = c.real == 0
        assert float(f.nf[pad][:, c.zero_cols].abs().max()) == 0.0, "nf is exactly 0 on a padded row's zero columns"
        assert float(f.nf[pad].abs().max()) > 0.0
    if c.layout == "64+32at128":
        assert float(f.pt[:, 64:128].abs().max()) == 0.0 and (float(f.pt[:, :64].abs().max()) > 0.0 or spec["pad"] == "allpad")
    y4, y2 = tr.saved_for_backward(c)
    if bool((c.real > 0).any()):
        assert bool((y4[c.real > 0] == 0).any()) and bool((y2[c.real > 0] == 0).any())


def test_the_matrix_covers_what_it_names():
    ids = [tr.spec_id(s) for s in ALL_SPECS]
    assert len(set(ids)) == len(ids)
    have = lambda specs, **kw: any(all(s.get(k) == v for k, v in kw.items()) for s in specs)  # noqa: E731
    fwd, bwd, asm, gat = tr.fwd_specs(), tr.bwd_specs(), tr.assemble_specs(), tr.gather_specs()
    for G, N in tr.FWD_SHAPES + ((1, 0), (17, 0)):
        assert have(fwd, G=G, N=N) and have(asm, entry="qkv", G=G, N=N, C=192) and have(asm, entry="qkv", G=G, N=N, C=256)
    for G, N in tr.BWD_SHAPES:
        assert have(bwd, G=G, N=N)
    for specs in (fwd, bwd):
        for d in tr.DROPOUTS:
            for m in ("whole", "split"):
                assert have(specs, drop=d, seed_mode=m)
        for p in tr.PADS:
            assert have(specs, pad=p)
    for lay in tr.LAYOUTS:
        for f in (0, 1, 3):
            assert have(fwd, layout=lay, n_fold=f) and have(gat, layout=lay, n_fold=f)
    for a in (1, 2, 4):
        assert have(fwd, n_add=a) and have(gat, n_add=a)
    for i in ("i64", "i32"):
        assert have(fwd, idx=i) and have(gat, idx=i)
    for a, b in tr.BWD_STRIDES:
        assert have(bwd, ld_y2=a, ld_dx4=b)
    for C in tr.ASSEMBLE_WIDTHS:
        for bf in ("bf16", "f32only"):
            assert have(asm, entry="assemble", C=C, bf16=bf)
        assert have(asm, entry="assemble", C=C, N=0, G=1) and have(asm, entry="assemble", C=C, N=0, G=17)
    for R in tr.GATHER_ROWS:
        assert have(gat, G=R)


# mutant -> which verdict sees it; every one on each of the smallest cases that has what the mutant needs
SMALL = [dict(G=2, N=7, n_fold=1), dict(G=4, N=3, n_fold=3), dict(G=3, N=5, n_fold=1)]
FWD_MUTANTS = ("no_keep_pos", "no_keep_in", "salts_swapped", "in_rows_gn", "w2_transposed", "w4_transposed", "kstep_f2", "kstep_nf",
               "kstep_qkv", "fold_dropped", "row_past_R")
BWD_MUTANTS = ("real_not_applied", "leaky_wrong_side", "w4_transposed_bwd", "w2_transposed_bwd", "kstep_dx4", "kstep_dpt",
               "d_token_overwritten", "row_past_R")
SCATTER_MUTANTS = ("extra_row0_row1", "padding_row_not_skipped")


def small_case(k):
    return tr.make_case(pad="mixed", p_pos=0.1, p_in=0.3, layout="128+32", n_add=4, **SMALL[k])


def verdict_forward(c, mut):
    b = tr.emulate_forward(c, mut)
    return tr.judge_forward(c, b.cpu()) + b.guard_failures()


def verdict_backward(c, mut):
    y4, y2 = tr.saved_for_backward(c)
    b = tr.emulate_backward(c, y4, y2, mut)
    return tr.judge_backward(c, b.cpu(), y4, y2) + b.guard_failures()


def verdict_scatter(c, mut):
    bk = tr.backward(c, tr.forward(c))
    bufs = {0: tr.f32r(bk.d_pt), 1: tr.f32r(bk.dx4), 2: tr.f32r(bk.d_add)}
    extra = tr.f32r(bk.d_token)
    got = tr.emulate_scatter(c, bufs, extra, mut)
    return tr.judge_scatter(c.jobs, bufs, got, extra_row0=extra, extra_job=tr.live_index(c, c.pos_job))


def test_every_mutant_has_a_verdict():
    assert set(FWD_MUTANTS) | set(BWD_MUTANTS) | set(SCATTER_MUTANTS) == set(tr.MUTANTS)


@pytest.mark.parametrize("k", range(len(SMALL)))
def test_a_correct_result_is_accepted(k):
    c = small_case(k)
    assert verdict_forward(c, None) == [] and verdict_backward(c, None) == [] and verdict_scatter(c, None) == []


@pytest.mark.parametrize("mut", tr.MUTANTS)
def test_mutants_are_rejected(mut):
    for k in range(len(SMALL)):
        c = small_case(k)
        seen = []
        if mut in FWD_MUTANTS:
            seen.append(verdict_forward(c, mut))
        if mut in BWD_MUTANTS:
            seen.append(verdict_backward(c, mut))
        if mut in SCATTER_MUTANTS:
            seen.append(verdict_scatter(c, mut))
        assert seen and all(seen), (mut, SMALL[k], "not rejected")


def test_masks_follow_the_three_numberings():
    """keep_in row g T + t and keep_nf row g N + n are rows of ONE stream per site: a batch's mask is a prefix-independent function of
    (seed, salt, row), and the three sites differ."""
    c = tr.make_case(3, 5, "mixed", 0.1, 0.3)
    whole = tr.site_keep(c.seed, c.salts[2], c.G * c.T, c.C, c.p_in)
    assert torch.equal(c.keep_in, torch.from_numpy(whole).to(F64))
    assert not torch.equal(c.keep_nf[:c.G], c.keep_tok)
    assert abs(tr.inv_keep_of(0.3) - 1.0 / (1.0 - 19661 / 65536.0)) < 1e-6
